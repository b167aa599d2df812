"""Raw-limb cases for the field, point and scalar arithmetic of elastic_elgamal_amd/csrc/{fe,ge,sc}25519.cuh, with their reference.

The field element of fe25519.cuh is 9 limbs of 29/28/28 bits whose additions and subtractions are not carried; the header's "bound
discipline" says how far each limb may grow ("class c": limb i <= c * 2^W(i)) before an operation.  Points and encodings never
drive a limb near the top of its class, so these cases inject limbs directly: every operation is run on limb vectors that sit on
the corners its precondition allows, and is compared with the mathematical operation on value(limbs) in Python integers.

* layout (W, POS, dbl, value) and `reference`: the operations on integers mod p / mod l.  No column code here.
* `model_mul` / `model_sq`: the column sums of fe_mul / fe_sq in unbounded integers, in the schedule of EG_FE_COLUMNS_LOW.  Used
  only to say how high a case drives the 64-bit accumulators and the final carry (tests/test_limb_corners_cpu.py), never as the
  expected result.
* `family`: the corner cases of a tuple of classes; `MATRIX`: the batches (operation x families) that the host bound-check build
  (tests/test_limb_corners_cpu.py) and the HIP build (tests/test_gpu_limb_corners.py) both run through tests/devcheck/limb_ops.cuh.

Record format (limb_ops.cuh): 80 input words (8 slots of 9 limbs + 8 extra words), 8 classes, 80 output words.
"""
import math
import random
import struct

import numpy as np

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
NL = 9
W = [29 if i % 3 == 0 else 28 for i in range(NL)]
POS = [(85 * i + 2) // 3 for i in range(NL)]
MASK = [(1 << w) - 1 for w in W]
P_LIMBS = [(1 << 29) - 19] + MASK[1:]                 # p itself, as fe_sub adds it (twice)
SLOTS, WORDS, EXTRA = 8, 80, 72
D = (-121665 * pow(121666, P - 2, P)) % P
D2 = 2 * D % P
SQRTM1 = pow(2, (P - 1) // 4, P)

# limb 1 of a class-1 result may exceed its 28 bits by what the final wrap of fe_mul / fe_sq adds to it: (limb 0 + 19 * carry) >> 29
# with carry < 2^36.  HAIR is the largest such addend the column model gives over every fe_mul / fe_sq case of MATRIX (reached at class
# product 12.5 with the slack of fe_check_values; the CPU test asserts the figure); HAIR_BOUND is the analytic bound for a 36-bit carry.
HAIR = 2142
HAIR_BOUND = ((1 << 29) - 1 + 19 * ((1 << 36) - 1)) >> 29

OPS = {name: i for i, name in enumerate(
    ["mul", "sq", "sqn", "add", "sub", "sub4", "neg", "carry", "canon", "from_words", "invert", "pow22523", "sqrt_ratio",
     "add_to_p3", "add_to_p2", "dbl_to_p3", "dbl_to_p2", "ge_add", "ge_madd", "ge_dbl", "to_cached", "to_cached_lazy",
     "cached_cneg", "niels_cneg", "sc_muladd", "sc_mul", "sc_add", "sc_from_wide", "sc_is_canonical", "sc_neg", "sc_halve"])}


def dbl(i, j):
    """the product of limbs i and j carries an extra factor 2 (fe_dbl)"""
    return (i % 3 == 1 and j % 3 != 0) or (i % 3 == 2 and j % 3 == 1)


def value(limbs):
    return sum(int(v) << p for v, p in zip(limbs, POS))


def f32(c):
    return struct.unpack("f", struct.pack("f", c))[0]


def top(c, i):
    """the largest limb i of class c: floor(c * 2^W(i)), c as the float the build carries"""
    return int(f32(c) * (1 << W[i]))


def slack_top(c, i):
    """the largest limb i that fe_check_values admits for class c (0.1 % + 4096 above the nominal bound)"""
    return min(int(float(1 << W[i]) * f32(c) * 1.001 + 4096.0), 2**32 - 1)


def slice_limbs(v):
    """the integer v cut at the limb positions: limbs 0..7 within their widths, the excess in limb 8"""
    return [(v >> POS[i]) & MASK[i] for i in range(NL - 1)] + [v >> POS[NL - 1]]


def in_class(limbs, c, slack=False):
    """class 1: what fe_mul / fe_sq / fe_carry promise (every limb within its width, limb 1 at most HAIR above); class c: limb i at
    most floor(c * 2^W(i)), limb 1 a hair above per unit of class.  slack: the result of an uncarried operation on inputs that use
    the slack of fe_check_values, which it inherits"""
    if c == 1 and not slack:
        return all(v <= MASK[i] + (HAIR if i == 1 else 0) for i, v in enumerate(limbs))
    extra = math.ceil(c) * (slack_top(1, 0) - top(1, 0)) if slack else 0
    return all(v <= top(c, i) + (math.ceil(c) * HAIR if i == 1 else 0) + extra for i, v in enumerate(limbs))


# ---- the column model ---------------------------------------------------------------------------------------------------------
def _columns_low(low_terms, hc):
    limbs, carry, peak = [0] * NL, 0, max(hc)
    for k in range(NL):
        acc = carry + low_terms(k)
        if k + NL < 2 * NL - 1:
            acc += (hc[k] & 0xFFFFFFFF) * 19
        if k >= 1:
            acc += ((hc[k - 1] >> 32) & 0xFFFFFFFF) * (19 << (32 - W[k - 1]))
        peak = max(peak, acc)
        limbs[k] = acc & MASK[k]
        carry = acc >> W[k]
    c0 = limbs[0] + 19 * carry
    limbs[0] = c0 & MASK[0]
    limbs[1] += c0 >> 29
    return limbs, peak, carry, c0 >> 29


def model_mul(f, g):
    """(limbs, largest column sum, final carry, what the wrap adds to limb 1) of fe_mul in unbounded integers"""
    f2 = [(2 * f[i]) & 0xFFFFFFFF if i % 3 else 0 for i in range(NL)]
    term = lambda i, j: (f2[i] if dbl(i, j) else f[i]) * g[j]
    hc = [sum(term(i, k - i) for i in range(k - NL + 1, NL)) for k in range(NL, 2 * NL - 1)]
    return _columns_low(lambda k: sum(term(i, k - i) for i in range(k + 1)), hc)


def model_sq(f):
    d = [(2 * v) & 0xFFFFFFFF for v in f]

    def col(k):
        acc = 0
        for i in range(NL):
            j = k - i
            if j < i or j >= NL:
                continue
            acc += (d[i] if dbl(i, i) else f[i]) * f[i] if i == j else d[i] * (d[j] if dbl(i, j) else f[j])
        return acc
    return _columns_low(col, [col(k) for k in range(NL, 2 * NL - 1)])


# ---- case families ------------------------------------------------------------------------------------------------------------
CORNER = ("top", "slack", "near", "hair")          # the families named for the corner of a class (pair)


def unreduced(c):
    """representations of 0 and of small values inside class c: k p + d, as limb-wise multiples of p (what fe_sub(x, x) and fe_sub4
    give) and cut at the limb positions (the excess in the top limb)"""
    out = []
    for k in (1, 2, 4):
        if k > c:
            continue
        for d in (-1, 0, 1):
            a = [k * v for v in P_LIMBS]
            a[0] += d
            out.append(a)
            b = slice_limbs(k * P + d)
            if b[NL - 1] <= top(c, NL - 1):
                out.append(b)
    return out


def family(classes, rng, total, additive_slack=True):
    """[(name, [limbs of operand 0, limbs of operand 1, ..])]: the corners of a tuple of classes, filled up to `total` with uniform
    random limbs within the classes.  additive_slack=False: the "slack" case takes the 0.1 % of fe_check_values without its + 4096,
    for formulas that add two inputs before they multiply (the sum of two + 4096 is outside the class of the sum)"""
    k = len(classes)
    tops = [[top(c, i) for i in range(NL)] for c in classes]
    rand = lambda o: [rng.randrange(tops[o][i] + 1) for i in range(NL)]
    out = [("top", [list(t) for t in tops]), ("slack", [[slack_top(c, i) - (0 if additive_slack else 4097) for i in range(NL)] for c in classes])]
    for _ in range(8):
        out.append(("near", [[max(0, v - rng.randrange(1 << rng.randrange(1, 13))) for v in t] for t in tops]))
    out.append(("hair", [[v + (math.ceil(c) * HAIR if i == 1 else 0) for i, v in enumerate(t)] for c, t in zip(classes, tops)]))
    for o in range(k):
        for i in range(NL):
            ops = [list(t) for t in tops]
            ops[o] = [tops[o][j] if j == i else 0 for j in range(NL)]
            out.append(("onehot", ops))
    if k == 2:
        for i in range(NL):
            for j in range(NL):
                out.append(("onehot2", [[tops[0][a] if a == i else 0 for a in range(NL)], [tops[1][a] if a == j else 0 for a in range(NL)]]))
    for ph in range(1 << min(k, 4)):
        out.append(("alternating", [[t[i] if (i + (ph >> (o % 4))) % 2 == 0 else 0 for i in range(NL)] for o, t in enumerate(tops)]))
    out.append(("zero", [[0] * NL for _ in classes]))
    for o, c in enumerate(classes):
        for u in unreduced(c):
            for other in ("top", "random"):
                ops = [list(t) if other == "top" else rand(q) for q, t in enumerate(tops)]
                ops[o] = u
                out.append(("unreduced", ops))
    if k >= 2:
        for u in unreduced(min(classes)):
            out.append(("unreduced", [list(u) for _ in classes]))
    while len(out) < total:
        out.append(("random", [rand(o) for o in range(k)]))
    return out


def representations(v, c, rng, n=6):
    """limb vectors of class <= c whose value is congruent to v: the cut of v (+ k p while it fits), limb-wise multiples of p added,
    and units moved down from a limb into the one below it"""
    out = []
    for k in range(int(c) + 1):
        b = slice_limbs(v + k * P)
        if all(x <= top(c, i) for i, x in enumerate(b)):
            out.append(b)
        a = [x + k * q for x, q in zip(slice_limbs(v), P_LIMBS)]
        if k and all(x <= top(c, i) for i, x in enumerate(a)):
            out.append(a)
    for base in list(out):
        for _ in range(n):
            a = list(base)
            for _ in range(rng.randrange(1, 6)):
                i = rng.randrange(NL - 1)
                room = (top(c, i) - a[i]) >> (POS[i + 1] - POS[i])
                t = min(room, a[i + 1])
                if t > 0:
                    t = rng.randrange(1, t + 1)
                    a[i] += t << (POS[i + 1] - POS[i])
                    a[i + 1] -= t
            out.append(a)
    return out


# ---- batches ------------------------------------------------------------------------------------------------------------------
class Batch:
    """n cases of one operation: `inp` (n x 80 uint32), `cls` (n x 8 float32), `names` (family of every case), `classes` (the class
    tuple of every case); check(out) compares an n x 80 output with the reference"""

    def __init__(self, name, op):
        self.name, self.op, self.rows, self.cl, self.names, self.classes = name, op, [], [], [], []

    def add(self, fam, classes, operands, extra=()):
        row = [0] * WORDS
        for s, limbs in enumerate(operands):
            row[NL * s : NL * s + NL] = limbs
        row[EXTRA : EXTRA + len(extra)] = extra
        self.rows.append(row)
        self.cl.append(list(classes) + [1.0] * (SLOTS - len(classes)))
        self.names.append(fam)
        self.classes.append(tuple(classes))

    def add_words(self, fam, words):
        self.rows.append(list(words) + [0] * (WORDS - len(words)))
        self.cl.append([1.0] * SLOTS)
        self.names.append(fam)
        self.classes.append(())

    def finish(self):
        assert len(self.rows) >= 4096 and len(self.rows) % 64 != 0, (self.name, len(self.rows))
        self.inp = np.array(self.rows, dtype=np.uint32)
        self.cls = np.array(self.cl, dtype=np.float32)
        return self

    def __len__(self):
        return len(self.rows)

    def check(self, out, rows=None):
        """out: the output records of the cases `rows` (default: all of them, in order)"""
        out = np.asarray(out).tolist()
        rows = range(len(self.rows)) if rows is None else rows
        assert len(out) == len(rows)
        for r, o in zip(rows, out):
            try:
                reference(self.name, self.rows[r], self.classes[r], o, self.names[r])
            except AssertionError as e:
                raise AssertionError(f"{self.name} case {r} ({self.names[r]}, classes {self.classes[r]}): {e}\n in  {self.rows[r]}\n out {o}") from None


def _slot(row, s):
    return row[NL * s : NL * s + NL]


def _words(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def _to_words(v, n=8):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def _expect_fe(o, s, want, c, what, slack=False):
    got = _slot(o, s)
    assert value(got) % P == want % P, f"{what}: value {value(got) % P:#x}, expected {want % P:#x}"
    assert in_class(got, c, slack), f"{what}: limbs {got} outside class {c}"


def sqrt_ratio_m1(u, v):
    """RFC 9496 4.2 on integers: (was_square, r)"""
    r = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    check = v * r * r % P
    correct, flipped, flipped_i = check == u % P, check == -u % P, check == -u * SQRTM1 % P
    if flipped or flipped_i:
        r = r * SQRTM1 % P
    if r & 1:
        r = P - r
    return correct or flipped, r


def reference(name, row, classes, o, fam=""):
    """asserts the output record o of one case against the operation on integers"""
    f, g = value(_slot(row, 0)), value(_slot(row, 1))
    x = row[EXTRA]
    if name in ("mul", "sq", "sqn", "add", "sub", "sub4", "neg", "carry"):
        cf, cg = classes[0], (classes[1] if len(classes) > 1 else 1)
        want, c = {"mul": (f * g, 1), "sq": (f * f, 1), "sqn": (pow(f, 2 ** x, P), 1), "add": (f + g, cf + cg), "sub": (f - g, cf + 2),
                   "sub4": (f - g, cf + 4), "neg": (-f, 2), "carry": (f, 1)}[name]
        _expect_fe(o, 0, want, c, "h", fam == "slack" and c != 1)
        assert _slot(o, 1) == _slot(o, 0), "h aliasing f differs"
        assert _slot(o, 2) == _slot(o, 0), "h aliasing g differs"
        assert _words(o[EXTRA:]) == want % P, "canonical words"
        if name in ("add", "sub", "sub4", "neg", "carry"):       # not reduced: the integer itself is determined
            exact = {"add": f + g, "sub": f + 2 * P - g, "sub4": f + 4 * P - g, "neg": 2 * P - f}.get(name)
            if exact is not None:
                assert value(_slot(o, 0)) == exact, "integer value"
    elif name == "canon":
        v = f % P
        assert _words(o[EXTRA:]) == v, f"fe_to_words {_words(o[EXTRA:]):#x}, expected {v:#x}"
        assert o[0] == (v & 1) and o[1] == int(v == 0), "isnegative / iszero"
        assert o[2] == o[3] == int(v == g % P), "fe_eq"
        if x:
            assert _words(o[NL : NL + 8]) == f, "fe_pack8"
            assert _slot(o, 2) == slice_limbs(f), "fe_unpack8"
    elif name == "from_words":
        v = _words(row[:8]) & (2**255 - 1)
        assert _slot(o, 0) == slice_limbs(v), "fe_from_words"
        assert _words(o[EXTRA:]) == v % P, "canonical words"
    elif name in ("invert", "pow22523"):
        want = pow(f, P - 2 if name == "invert" else (P - 5) // 8, P)
        _expect_fe(o, 0, want, 1, name)
        assert _words(o[EXTRA:]) == want
    elif name == "sqrt_ratio":
        sq, r = sqrt_ratio_m1(f, g)
        _expect_fe(o, 0, r, 1, "r")
        assert _words(o[EXTRA:]) == r and o[NL] == int(sq), "root / was_square"
        assert r & 1 == 0
        if g % P:                                              # the defining property, independent of the steps above
            assert g * r * r % P == (f if sq else f * SQRTM1) % P
        else:
            assert r == 0 and sq == (f % P == 0)
    elif name in ("add_to_p3", "add_to_p2", "dbl_to_p3", "dbl_to_p2"):
        X, Y, Z, T = (value(_slot(row, s)) for s in range(4))
        _expect_fe(o, 0, X * T, 1, "X")
        _expect_fe(o, 1, Y * Z, 1, "Y")
        _expect_fe(o, 2, Z * T, 1, "Z")
        if name.endswith("p3"):
            _expect_fe(o, 3, X * Y, 1, "T")
        else:
            assert _slot(o, 3) == [0] * NL
    elif name in ("ge_add", "ge_madd", "ge_dbl"):
        X1, Y1, Z1, T1 = (value(_slot(row, s)) for s in range(4))
        if name == "ge_dbl":
            xx, yy, b2, aa = X1 * X1, Y1 * Y1, 2 * Z1 * Z1, (X1 + Y1) ** 2
            H, G = yy + xx, yy - xx
            E, F = aa - H, b2 - G
            out_cls = (5, 2, 3, 1)
        else:
            ypx, ymx = value(_slot(row, 4)), value(_slot(row, 5))
            if name == "ge_madd":                              # affine entry (y+x, y-x, 2dxy): D = 2 Z1
                t2d, dd, out_cls = value(_slot(row, 6)), 2 * Z1, (3, 2, 3, 4)
            else:                                              # cached entry (Y+X, Y-X, 2Z, 2dT): D = Z1 * 2Z2
                t2d, dd, out_cls = value(_slot(row, 7)), Z1 * value(_slot(row, 6)), (3, 2, 2, 3)
            if x == 2:                                         # the addend negated: -(x, y) = (-x, y)
                ypx, ymx, t2d = ymx, ypx, -t2d
            pp, mm, tt = (Y1 + X1) * ypx, (Y1 - X1) * ymx, T1 * t2d
            E, H, G, F = pp - mm, pp + mm, dd + tt, dd - tt
        for s, (want, c, what) in enumerate(zip((E, H, G, F), out_cls, "EHGF")):
            _expect_fe(o, s, want, c, what)
        for s, (want, what) in enumerate(zip((E * F, G * H, F * G, E * H), "XYZT")):
            _expect_fe(o, 4 + s, want, 1, what + "3")
    elif name in ("to_cached", "to_cached_lazy"):
        X, Y, Z, T = (value(_slot(row, s)) for s in range(4))
        lazy = name == "to_cached_lazy"
        out_cls = (classes[1] + classes[0], classes[1] + 2, 2 * classes[2], 1) if lazy else (1, 1, 1, 1)
        for s, (want, c, what) in enumerate(zip((Y + X, Y - X, 2 * Z, T * D2), out_cls, ("YpX", "YmX", "Z2", "T2d"))):
            _expect_fe(o, s, want, c, what, fam == "slack" and c != 1)
    elif name in ("cached_cneg", "niels_cneg"):
        ts, n = (3, 4) if name == "cached_cneg" else (2, 3)     # slot of T2d / xy2d, slots of the entry
        if x:
            assert _slot(o, 0) == _slot(row, 1) and _slot(o, 1) == _slot(row, 0), "Y+X and Y-X not swapped"
            assert value(_slot(o, ts)) == 2 * P - value(_slot(row, ts)) and in_class(_slot(o, ts), 2), "negated T"
            if n == 4:
                assert _slot(o, 2) == _slot(row, 2), "Z changed"
        else:
            assert o[: NL * n] == row[: NL * n], "entry changed by cneg(false)"
    else:
        a, b, c = _words(row[0:8]), _words(row[9:17]), _words(row[18:26])
        got = _words(o[:8])
        if name == "sc_halve":
            assert 2 * got % L == a % L and got < 2**252 + 2**251, f"sc_halve {got:#x}"
        else:
            want = {"sc_muladd": lambda: (a * b + c) % L, "sc_mul": lambda: a * b % L, "sc_add": lambda: (a + b) % L,
                    "sc_from_wide": lambda: _words(row[0:16]) % L, "sc_is_canonical": lambda: int(a < L), "sc_neg": lambda: -a % L}[name]()
            assert got == want, f"{name}: {got:#x}, expected {want:#x}"
        assert o[8:] == [0] * (WORDS - 8)


MUL_PAIRS = [(1, 1), (2, 3), (3, 2), (4, 3), (3, 4), (3.5, 3.5), (5, 2), (7.9, 1.58), (1.58, 7.9), (6.25, 2), (5, 2.5), (2.5, 5),
             (5, 1), (3, 1), (3, 3), (2, 2), (4, 2), (2, 1), (3, 3.3)]    # from (5, 1): the pairs of ge_dbl_to_p3 / ge_add_to_p3 / ge_add
SQ_CLASSES = [1, 2, 3, 3.5]
TOTAL = 4096 + 37
SC_EDGE = [0, 1, L - 1, L, L + 1, 2**252, 2**253 - 1, 2**256 - 1]
CANON_VALUES = [0, 1, 19, P - 1, P, P + 1, 2 * P, 2 * P - 1, 2 * P + 1, 2**255 - 1, 2**255, 2**255 + 2**41, 2**255 - 20, 2**255 - 18]


def _spread(b, tuples, rng, extra=lambda i: (), per_min=0, additive_slack=True):
    """the families of each class tuple, the random fill shared out so that the batch holds at least TOTAL cases"""
    per = max(-(-TOTAL // len(tuples)), per_min)
    for classes in tuples:
        for fam, ops in family(classes, rng, per, additive_slack):
            b.add(fam, classes, ops, extra(len(b)))
    while len(b) % 64 == 0 or len(b) < TOTAL:
        classes = tuples[len(b) % len(tuples)]
        b.add("random", classes, [[rng.randrange(top(c, i) + 1) for i in range(NL)] for c in classes], extra(len(b)))
    return b.finish()


def _build(name):
    rng = random.Random("limb-cases-" + name)
    b = Batch(name, OPS[name])
    if name == "mul":
        return _spread(b, MUL_PAIRS, rng, per_min=330)
    if name == "sq":
        return _spread(b, [(c,) for c in SQ_CLASSES], rng)
    if name == "sqn":
        return _spread(b, [(c,) for c in SQ_CLASSES], rng, lambda i: (2 if i % 2 else 5,))
    if name == "add":
        return _spread(b, [(1, 1), (3.9, 4), (4, 3.9), (1, 6.9), (6.9, 1), (2, 3), (3.95, 3.95)], rng)
    if name == "sub":
        return _spread(b, [(1, 1), (0, 1), (2, 1), (3, 1), (5.9, 1)], rng)
    if name == "sub4":
        return _spread(b, [(1, 1), (1, 2), (2, 3), (1, 3.9), (3.9, 3.9), (3.9, 1)], rng)
    if name == "neg":
        return _spread(b, [(1,)], rng)
    if name == "carry":
        return _spread(b, [(1,), (2,), (3,), (5,), (6,), (7.9,)], rng)
    if name == "canon":
        for c in (1, 2, 3, 4, 5.9, 7.9):
            reps = [(v, r) for v in CANON_VALUES for r in representations(v, c, rng)]
            for v, r in reps:
                for w in (v, v + 1, rng.randrange(P)):            # g: an equal value in another representation, a neighbour, anything
                    gs = representations(w % (2**255 + 2**41), c, rng, 1)
                    b.add("value", (c, c), [r, gs[rng.randrange(len(gs))]], (int(c == 1),))
            for fam, ops in family((c, c), rng, 160):
                b.add(fam, (c, c), ops, (int(c == 1 and fam != "slack"),))      # fe_pack8 takes class 1 proper: limb 8 <= 2^28
        return _spread(b, [(1, 1), (7.9, 7.9), (3, 5)], rng, lambda i: (0,))
    if name == "from_words":
        vals = CANON_VALUES + [2**256 - 1, 2**255 + 19, 2**256 - 38, 2**29 - 1, 2**57 - 1, 2**227, 2**228 - 1]
        vals += [(1 << POS[i]) - 1 for i in range(1, NL)] + [1 << POS[i] for i in range(1, NL)]
        for v in vals:
            b.add_words("edge", _to_words(v))
        while len(b) < TOTAL:
            b.add_words("random", _to_words(rng.getrandbits(256)))
        return b.finish()
    if name in ("invert", "pow22523"):
        return _spread(b, [(1,), (2,), (3.5,)], rng)
    if name == "sqrt_ratio":
        for _ in range(300):
            s, v = rng.randrange(P), rng.randrange(1, P)
            for u in (s * s * v % P, SQRTM1 * s * s * v % P, 2 * s * s * v % P, -s * s * v % P, 0, s):
                b.add("ratio", (1, 1), [slice_limbs(u), slice_limbs(v)])
            b.add("v=0", (1, 1), [slice_limbs(s), [0] * NL])
            b.add("v=p", (1, 1), [slice_limbs(s), list(P_LIMBS)])
        b.add("0/0", (1, 1), [[0] * NL, [0] * NL])
        return _spread(b, [(1, 1)], rng)
    if name in ("add_to_p3", "add_to_p2"):
        return _spread(b, [(3, 2, 3, 4), (3, 2, 2, 3), (3, 2, 2, 4), (3, 2, 3, 3)], rng)
    if name in ("dbl_to_p3", "dbl_to_p2"):
        return _spread(b, [(5, 2, 3, 1)], rng)
    if name == "ge_add":                                        # addend: a carried entry, a lazily stored one (ge_to_cached_lazy)
        return _spread(b, [(1, 1, 1, 1, 1, 1, 1, 1), (1, 1, 1, 1, 2, 3, 2, 1)], rng, lambda i: (i % 3,), additive_slack=False)
    if name == "ge_madd":
        return _spread(b, [(1, 1, 1, 1, 1, 1, 1)], rng, lambda i: (i % 3,), additive_slack=False)
    if name == "ge_dbl":
        return _spread(b, [(1, 1, 1), (1, 1, 2), (1, 1, 3.5), (1.75, 1.75, 3.5)], rng, additive_slack=False)
    if name == "to_cached":
        return _spread(b, [(1, 1, 1, 1)], rng, additive_slack=False)
    if name == "to_cached_lazy":
        return _spread(b, [(1, 1, 1, 1), (1, 1, 2, 1)], rng, additive_slack=False)
    if name == "cached_cneg":
        return _spread(b, [(1, 1, 1, 1), (2, 3, 2, 1)], rng, lambda i: (i % 2,))
    if name == "niels_cneg":
        return _spread(b, [(1, 1, 1)], rng, lambda i: (i % 2,))
    # scalars
    row = lambda a, bb=0, c=0: _to_words(a) + [0] + _to_words(bb) + [0] + _to_words(c)
    if name in ("sc_muladd", "sc_mul", "sc_add"):
        for a in SC_EDGE:
            for bb in SC_EDGE:
                for c in SC_EDGE:
                    b.add_words("edge", row(a, bb, c))
        while len(b) < TOTAL:
            pick = lambda: rng.choice(SC_EDGE) if rng.random() < 0.2 else rng.getrandbits(256) if rng.random() < 0.5 else rng.randrange(L)
            b.add_words("random", row(pick(), pick(), pick()))
    elif name == "sc_from_wide":
        for v in [2**512 - 1, 0, L, L - 1, L << 256, (L << 259) - 1, 2**512 - 2**256, 2**504 - 1] + [e << s for e in SC_EDGE for s in (0, 128, 256)]:
            b.add_words("edge", _to_words(v, 16))
        while len(b) < TOTAL:
            b.add_words("random", _to_words(rng.getrandbits(512), 16))
    elif name == "sc_is_canonical":
        for v in SC_EDGE + [L - 2, L + 2**32, L - 2**32, L ^ (1 << 128), 2**255]:
            b.add_words("edge", row(v))
        while len(b) < TOTAL:
            v = rng.choice([rng.getrandbits(256), rng.randrange(L), L + rng.randrange(-2**20, 2**20), L ^ (1 << rng.randrange(256))])
            b.add_words("random", row(v))
    else:                                                       # sc_neg, sc_halve: canonical operands only, as their comments require
        for v in [0, 1, 2, 3, L - 1, L - 2, L - 3, 2**252, 2**252 - 1, 2**252 + 1]:
            b.add_words("edge", row(v))
        while len(b) < TOTAL:
            b.add_words("random", row(rng.randrange(L)))
    return b.finish()


MATRIX = list(OPS)                    # every operation; batch(name) makes its cases (deterministic, cached)
_cache = {}


def batch(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]
