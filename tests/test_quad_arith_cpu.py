"""The quad-lane point arithmetic (elastic_elgamal_amd/csrc/ge25519_quad.cuh) in its bound-check host build
(tests/hostcheck/quadcheck.cpp: -DEG_BOUNDCHECK under UBSan, a quad emulated as an array of four lanes).

Every quad operation is compared with the one-lane operation of ge25519.cuh and with Python integers on the limb-corner inputs of
tests/limb_cases.py and on random points; whole products (the comb table a quad builds, the product over it, the fixed-base comb) are
compared with the oracle's scalar multiplication on edge scalars.  A case outside a documented precondition trips the bound assertion.
"""
import ctypes as C
import os
import random
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import limb_cases as lc  # noqa: E402

P, L, NL = lc.P, lc.L, lc.NL
D2 = 2 * lc.D % P
OP = {"dbl": 0, "add": 1, "madd": 2, "to_cached": 3, "cached_cneg": 4, "neg": 5, "cached_to_p2": 6, "identity": 7, "dbl_wide": 8,
      "cached_to_p3": 9, "cached_neg_t": 10, "cached_identity": 11, "from_cached": 12}
SRC = HERE / "hostcheck" / "quadcheck.cpp"
LIB = HERE / "hostcheck" / "libquadcheck.so"
CMD = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DEG_BOUNDCHECK", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def qc():
    srcs = [SRC, HERE / "quaddev" / "quad_ops.cuh"] + list((HERE.parent / "elastic_elgamal_amd" / "csrc").glob("*.cuh"))
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in srcs):
        subprocess.check_call(CMD + os.environ.get("EG_HOSTCHECK_FLAGS", "").split() + ["-o", str(LIB), str(SRC)])
    return C.CDLL(str(LIB))


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o

    o.build()
    return o


Arr = (C.c_uint32 * NL) * 4
Cls = C.c_float * 4


def run_op(qc, op, a, ca, b=None, cb=None):
    """-> (quad result, one-lane result), four limb vectors each in the one-lane order"""
    b = b or [[0] * NL] * 4
    cb = cb or [1.0] * 4
    A, B, oq, ol = Arr(), Arr(), Arr(), Arr()
    for i in range(4):
        for j in range(NL):
            A[i][j], B[i][j] = a[i][j], b[i][j]
    assert qc.qc_op(OP[op], A, Cls(*ca), B, Cls(*cb), oq, ol) == 1
    return [list(x) for x in oq], [list(x) for x in ol]


def val(limbs):
    return lc.value(limbs) % P


def want(op, a, b):
    """the operation over Python integers: coordinates mod p, in the one-lane order"""
    A = [val(x) for x in a]
    B = [val(x) for x in b] if b else None
    if op in ("dbl", "dbl_wide"):
        X, Y, Z = A[:3]
        E, H, G = 2 * X * Y, Y * Y + X * X, Y * Y - X * X
        F = 2 * Z * Z - G
        return [E * F % P, G * H % P, G * F % P, E * H % P]
    if op in ("add", "madd"):
        X, Y, Z, T = A
        z2 = 2 if op == "madd" else B[2]
        PP, MM, TT, DD = (Y + X) * B[0], (Y - X) * B[1], T * B[3], Z * z2
        E, H, G, F = PP - MM, PP + MM, DD + TT, DD - TT
        return [E * F % P, G * H % P, G * F % P, E * H % P]
    if op == "to_cached":
        X, Y, Z, T = A
        return [(Y + X) % P, (Y - X) % P, 2 * Z % P, D2 * T % P]
    if op == "cached_cneg":
        return [A[1], A[0], A[2], -A[3] % P]
    if op == "neg":
        return [-A[0] % P, A[1], A[2], -A[3] % P]
    if op == "cached_to_p2":
        return [(A[0] - A[1]) % P, (A[0] + A[1]) % P, A[2], None]
    if op == "identity":
        return [0, 1, 1, 0]
    if op == "cached_to_p3":          # (2X : 2Y : 2Z : 2T) of the point the addend is
        return [(A[0] - A[1]) % P, (A[0] + A[1]) % P, A[2], A[3] * pow(lc.D, P - 2, P) % P]
    if op == "cached_neg_t":
        return [A[0], A[1], A[2], -A[3] % P]
    if op == "cached_identity":
        return [1, 1, 2, 0]
    if op == "from_cached":
        return A
    raise KeyError(op)


# the classes every operation documents for its operands (ge25519_quad.cuh, header): the corners of these tuples are the cases
CLASSES = {
    "dbl": ((1.5, 2, 3, 1), None),          # what ge_dbl admits as well: it squares X + Y, class <= 3.5
    "dbl_wide": ((3, 3, 3, 1), None),       # what the quad admits: no sum is squared
    "add": ((1, 1, 1, 1), (3, 3, 3, 3)),
    "madd": ((1, 1, 1, 1), (3, 3, 1, 3)),
    "to_cached": ((1, 1, 1, 1), None),
    "cached_cneg": ((1, 1, 1, 1), None),
    "neg": ((1, 1, 1, 1), None),
    "cached_to_p2": ((3, 3, 3, 1), None),
    "identity": ((3, 3, 3, 3), None),
    "cached_to_p3": ((3, 3, 3, 3), None),   # "accepts the lazily stored classes (<= 3)"
    "cached_neg_t": ((1, 1, 1, 1), None),
    "cached_identity": ((3, 3, 3, 3), None),
    "from_cached": ((3, 3, 3, 3), None),
}


def check(qc, op, a, ca, b=None, cb=None, same_as_lane=True):
    got_q, got_l = run_op(qc, op, a, ca, b, cb)
    w = want(op, a, b)
    for i in range(4):
        if w[i] is None:
            continue
        assert val(got_q[i]) == w[i], (op, i, "quad vs integers")
        if same_as_lane:
            assert val(got_l[i]) == w[i], (op, i, "one lane vs integers")
    # what the next quad operation relies on: products come back in class 1
    if op in ("dbl", "dbl_wide", "add", "madd", "to_cached", "cached_to_p3"):
        for i in range(4):
            assert lc.in_class(got_q[i], 1), (op, i, got_q[i])


@pytest.mark.parametrize("op", list(OP))
def test_quad_operation_at_the_limb_corners(qc, op):
    """every corner family of tests/limb_cases.py for the classes the operation admits, filled up with random limbs"""
    rng = random.Random(OP[op] + 100)
    ca, cb = CLASSES[op]
    classes = list(ca) + list(cb or ())
    fam = lc.family(classes, rng, 700, additive_slack=False)
    names = set()
    for name, operands in fam:
        # the "hair" corner puts limb 1 above the class of a CARRIED value: it belongs to class-1 operands only, where it is part of the class
        if name == "hair" and any(c != 1 for c in classes):
            operands = [o if c == 1 else [min(v, lc.top(c, i)) for i, v in enumerate(o)] for o, c in zip(operands, classes)]
        if name == "slack" and op in ("cached_cneg", "neg", "to_cached", "add", "madd", "cached_neg_t"):
            continue        # these subtract a class-1 value limb by limb: the slack above the class is outside fe_sub's contract
        a, b = operands[:4], (operands[4:] if cb else None)
        check(qc, op, a, [float(c) for c in ca], b, [float(c) for c in cb] if cb else None)
        names.add(name)
    assert {"top", "near", "onehot", "alternating", "zero", "unreduced", "random"} <= names


def _point(rng):
    """a random point of the curve in extended coordinates with a random Z, as integers"""
    while True:
        y = rng.randrange(P)
        u, v = (y * y - 1) % P, (lc.D * y * y + 1) % P
        x2 = u * pow(v, P - 2, P) % P
        x = pow(x2, (P + 3) // 8, P)
        if (x * x - x2) % P:
            x = x * pow(2, (P - 1) // 4, P) % P
        if (x * x - x2) % P:
            continue
        z = rng.randrange(1, P)
        return [x * z % P, y * z % P, z, x * y % P * z % P]


def _affine(p):
    zi = pow(p[2], P - 2, P)
    return (p[0] * zi % P, p[1] * zi % P)


def _edwards_add(a, b):
    (x1, y1), (x2, y2) = a, b
    k = lc.D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + k, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - k, P - 2, P) % P)


def test_quad_operations_on_random_points_are_the_group_law(qc):
    """as projective points: quad doubling and addition of curve points equal the affine Edwards group law over Python integers, and the
    one-lane operations give the same point"""
    rng = random.Random(77)
    one = [1.0] * 4
    for _ in range(60):
        p, q = _point(rng), _point(rng)
        pl, ql = [lc.slice_limbs(v) for v in p], [lc.slice_limbs(v) for v in q]
        got_q, got_l = run_op(qc, "dbl", pl, one)
        for got in (got_q, got_l):
            g = [val(x) for x in got]
            assert _affine(g) == _edwards_add(_affine(p), _affine(p))
            assert g[3] * g[2] % P == g[0] * g[1] % P
        cq, _ = run_op(qc, "to_cached", ql, one)
        got_q, got_l = run_op(qc, "add", pl, one, cq, one)
        for got in (got_q, got_l):
            g = [val(x) for x in got]
            assert _affine(g) == _edwards_add(_affine(p), _affine(q))
            assert g[3] * g[2] % P == g[0] * g[1] % P
        # the negated addend subtracts
        nq, _ = run_op(qc, "cached_cneg", cq, one)
        got_q, _ = run_op(qc, "add", pl, one, nq, [1.0, 1.0, 1.0, 3.0])
        qa = _affine(q)
        assert _affine([val(x) for x in got_q]) == _edwards_add(_affine(p), ((-qa[0]) % P, qa[1]))


def _sc(x):
    return (x % L).to_bytes(32, "little")


def _edge_scalars():
    sys.path.insert(0, str(HERE.parent))
    import edge_ballots as eb

    return [0, 1, 2, L - 1, L - 2, 2**252, (L + 1) // 2, (L - 1) // 2] + list(eb.corner_scalars())


@pytest.mark.parametrize("teeth", [5, 6, 7])
def test_quad_products_equal_the_oracle_on_edge_scalars(qc, oracle, teeth):
    """[k]P + [r]G: table built by a quad, product by a quad (and by one lane over the quad's table: the layouts agree), fixed-base comb
    by a quad, against the oracle's vartime_double_mul_generator; 0, 1, l - 1 and the comb-digit corners in both positions"""
    rng = random.Random(500 + teeth)
    edge = _edge_scalars()
    pts = [oracle.point_mul_generator(_sc(s)) for s in (1, 2, L - 1, rng.randrange(1, L), rng.randrange(1, L))] + [bytes(32)]
    cases = [(k, r) for k in edge[:12] for r in edge[:12]]
    stride = {5: 1, 6: 2, 7: 7}[teeth]      # the long corner list: every scalar with 5 teeth (the choice ballots' shape), a stride otherwise
    cases += [(k, edge[(i * 7) % len(edge)]) for i, k in enumerate(edge[::stride])]
    cases += [(edge[(i * 5) % len(edge)], r) for i, r in enumerate(edge[::stride])]
    cases += [(rng.randrange(L), rng.randrange(L)) for _ in range(20)]
    out = C.create_string_buffer(32)
    for i, (k, r) in enumerate(cases):
        p = pts[i % len(pts)]
        assert qc.qc_double_mul_generator(teeth, _sc(k), p, _sc(r), 0, out) == 1
        w = oracle.point_double_mul_generator(_sc(k), p, _sc(r))
        assert out.raw == w, (teeth, k, r, "quad product")
        if i % 9 == 0:
            assert qc.qc_double_mul_generator(teeth, _sc(k), p, _sc(r), 1, out) == 1
            assert out.raw == w, (teeth, k, r, "one lane over the quad's table")


@pytest.mark.parametrize("teeth", [5, 6])
def test_quad_table_of_a_sum_of_bases(qc, oracle, teeth):
    """the comb table of B_1 + .. + B_m made from the members' tables without a doubling (quad_teeth_tables_sum): products over it equal
    the oracle's [k](sum) + [r]G, for members that cancel, the identity among them and a single member"""
    rng = random.Random(900 + teeth)
    pt = lambda s: oracle.point_mul_generator(_sc(s))
    a, b = rng.randrange(1, L), rng.randrange(1, L)
    groups = [[pt(a)], [pt(a), pt(b)], [pt(a), pt(L - a)], [bytes(32), pt(b), pt(1)], [pt(rng.randrange(1, L)) for _ in range(5)],
              [pt(a), pt(L - a), pt(b), pt(L - b)], [pt(1)] * 8]
    out = C.create_string_buffer(32)
    for members in groups:
        total = members[0]
        for m in members[1:]:
            total = oracle.point_add(total, m)
        for k, r in [(0, 0), (1, 0), (L - 1, 1), (rng.randrange(L), rng.randrange(L)), (2, L - 1)]:
            for lane in (0, 1):
                assert qc.qc_sum_mul_generator(teeth, _sc(k), b"".join(members), len(members), _sc(r), lane, out) == 1
                assert out.raw == oracle.point_double_mul_generator(_sc(k), total, _sc(r)), (len(members), k, r, lane)


def test_quad_fixed_base_comb_from_the_identity(qc, oracle):
    out = C.create_string_buffer(32)
    edge = _edge_scalars()
    for r in edge[:: max(1, len(edge) // 150)] + [0, 1, L - 1]:
        assert qc.qc_mul_generator(_sc(r), out) == 1
        assert out.raw == oracle.point_mul_generator(_sc(r)), r


_VIOLATION = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1])
Arr = (C.c_uint32 * 9) * 4
a, b, oq, ol = Arr(), Arr(), Arr(), Arr()
op, ca, cb = {"dbl4": (0, [4, 4, 4, 1], [1] * 4), "add_point2": (1, [2, 2, 2, 2], [1] * 4), "add_addend5": (1, [1] * 4, [5, 5, 5, 5])}[sys.argv[2]]
lib.qc_op(op, a, (C.c_float * 4)(*ca), b, (C.c_float * 4)(*cb), oq, ol)
print("survived")
"""


@pytest.mark.parametrize("case", ["dbl4", "add_point2", "add_addend5"])
def test_precondition_violation_trips_the_bound_assertion(qc, case):
    """a doubling of class-4 coordinates (4 x 4 > 12.5), an addition to a point that is not class 1 (fe_sub's subtrahend) and an addend of
    class 5 (3 x 5 > 12.5) are outside the documented preconditions: the build aborts with a bound violation"""
    r = subprocess.run([sys.executable, "-c", _VIOLATION, str(LIB), case], capture_output=True, text=True)
    assert r.returncode != 0 and "survived" not in r.stdout
    assert "bound violation" in r.stderr
