"""Cases for the fused square-and-subtract (fe_sq2_sub), the chain doubling (ge_dbl_chain, ge_dbl_chain_sgn), the comb product with
the sign on the accumulator (ge_teeth_mul) and the fixed comb's zero-digit path (ge_fixed_mul_add), with their reference on Python
integers.  Shared by tests/test_dbl_chain_cpu.py (stand-alone bound-check + sanitizer program tests/hostcheck/dblchaincheck.cpp) and
tests/test_gpu_dbl_chain.py (test-only device library tests/dblchaindev); the record format and the case families are those of
tests/limb_cases.py (tests/dblchaindev/chain_ops.cuh is the calling convention).

Class limits.  fe_sq2_sub(h, f, g) = 2 f^2 + 4p - g accumulates the columns of fe_sq doubled, i.e. those of fe_mul at class product
2 class(f)^2.  The header's column bound 0.078125 * class(f) * class(g) * 2^64 with the admitted product 12.5 gives 2 class(f)^2 <= 12.5:
F_LIMIT = 2.5 (0.9766 * 2^64 with every limb at the top; `model_sq2_sub` evaluates the columns in unbounded integers and the CPU test
asserts that the cases at 2.5 stay below 2^64 while the all-top case at 2.6 does not).  g is below class 4, as in fe_sub4: G_LIMIT = 3.9.
"""
import random

import numpy as np

import limb_cases as lc

P, L, NL = lc.P, lc.L, lc.NL
F_LIMIT, G_LIMIT = 2.5, 3.9
OPS = {"sq2_sub": 0, "dbl_chain": 1}
SQ2_PAIRS = [(F_LIMIT, G_LIMIT), (F_LIMIT, 1), (1, G_LIMIT), (2, 3), (1, 1), (2, G_LIMIT), (F_LIMIT, 3)]
# (X, Y, Z, flag): flag 0 / 1 = ge_dbl_chain_sgn(negx = false / true), X of class 1; flag 2 = ge_dbl_chain, X and Y as ge_dbl takes them
DBL_TUPLES = [((1, 1, 1), 0), ((1, 1, 2), 0), ((1, 1, F_LIMIT), 0), ((1, 1, 1), 1), ((1, 1, 2), 1), ((1, 1, F_LIMIT), 1),
              ((1, 1, 1), 2), ((1, 1, 2), 2), ((1, 1, F_LIMIT), 2), ((1.75, 1.75, F_LIMIT), 2)]
PER_TUPLE = 260


def model_sq2_sub(f, g):
    """(limbs, largest column sum, final carry, what the wrap adds to limb 1) of fe_sq2_sub in unbounded integers"""
    d = [(2 * v) & 0xFFFFFFFF for v in f]
    q = [(4 * v) & 0xFFFFFFFF for v in f]
    s = [(4 << lc.W[i]) - (76 if i == 0 else 4) - g[i] for i in range(NL)]

    def col(k):
        acc = 0
        for i in range(NL):
            j = k - i
            if j < i or j >= NL:
                continue
            acc += d[i] * (d[i] if lc.dbl(i, i) else f[i]) if i == j else d[i] * (q[j] if lc.dbl(i, j) else d[j])
        return acc
    return lc._columns_low(lambda k: s[k] + col(k), [col(k) for k in range(NL, 2 * NL - 1)])


class Batch:
    def __init__(self, name):
        self.name, self.op, self.rows, self.cl, self.names, self.classes = name, OPS[name], [], [], [], []

    def add(self, fam, classes, operands, flag=0):
        row = [0] * lc.WORDS
        for s, limbs in enumerate(operands):
            row[NL * s : NL * s + NL] = limbs
        row[lc.EXTRA] = flag
        self.rows.append(row)
        self.cl.append(list(classes) + [1.0] * (lc.SLOTS - len(classes)))
        self.names.append(fam)
        self.classes.append(tuple(classes))

    def finish(self):
        assert len(self.rows) % 64 != 0 and len(self.rows) > 256          # several blocks and a partial last wavefront
        self.inp = np.array(self.rows, dtype=np.uint32)
        self.cls = np.array(self.cl, dtype=np.float32)
        return self

    def __len__(self):
        return len(self.rows)

    def records(self):
        """the input file of `dblchaincheck records`: per case 80 words and 8 float classes"""
        return b"".join(self.inp[r].tobytes() + self.cls[r].tobytes() for r in range(len(self.rows)))

    def check(self, out):
        out = np.asarray(out).tolist()
        assert len(out) == len(self.rows)
        for r, o in enumerate(out):
            try:
                reference(self.name, self.rows[r], o)
            except AssertionError as e:
                raise AssertionError(f"{self.name} case {r} ({self.names[r]}, classes {self.classes[r]}): {e}\n in  {self.rows[r]}\n out {o}") from None


def reference(name, row, o):
    slot = lambda rec, s: rec[NL * s : NL * s + NL]
    val = lambda rec, s: lc.value(slot(rec, s))
    if name == "sq2_sub":
        f, g = val(row, 0), val(row, 1)
        want = (2 * f * f - g) % P
        got = slot(o, 0)
        assert lc.value(got) % P == want, f"value {lc.value(got) % P:#x}, expected {want:#x}"
        assert lc.in_class(got, 1), f"limbs {got} outside class 1"
        assert slot(o, 1) == got, "h aliasing f differs"
        assert slot(o, 2) == got, "h aliasing g differs"
        assert lc._words(o[lc.EXTRA:]) == want, "canonical words"
    else:
        X, Y, Z, flag = val(row, 0), val(row, 1), val(row, 2), row[lc.EXTRA]
        if flag == 1:
            X = -X
        xx, yy = X * X, Y * Y
        H, G = yy + xx, yy - xx
        E, F = (X + Y) ** 2 - H, 2 * Z * Z - G
        for s, (want, c, what) in enumerate(zip((E, H, G, F), (5, 2, 3, 1), "EHGF")):
            got = slot(o, s)
            assert lc.value(got) % P == want % P, f"{what}: value {lc.value(got) % P:#x}, expected {want % P:#x}"
            assert lc.in_class(got, c), f"{what}: limbs {got} outside class {c}"
            plain = lc.value(slot(o, 4 + s)) % P                 # ge_dbl on the same (X, Y, Z): equal on every coordinate mod p
            assert plain == (-want if flag == 1 and what == "E" else want) % P, f"{what}: ge_dbl gives {plain:#x}"
        assert lc.in_class(slot(o, 7), 1)


_cache = {}


def batch(name):
    if name in _cache:
        return _cache[name]
    rng = random.Random("dbl-chain-cases-" + name)
    b = Batch(name)
    if name == "sq2_sub":
        for classes in SQ2_PAIRS:
            for fam, ops in lc.family(classes, rng, PER_TUPLE):
                b.add(fam, classes, ops)
    else:
        for classes, flag in DBL_TUPLES:
            for fam, ops in lc.family(classes, rng, PER_TUPLE, additive_slack=False):
                b.add(fam, classes, ops, flag)
    while len(b) % 64 == 0:
        classes = SQ2_PAIRS[0] if name == "sq2_sub" else DBL_TUPLES[0][0]
        b.add("random", classes, [[rng.randrange(lc.top(c, i) + 1) for i in range(NL)] for c in classes])
    _cache[name] = b.finish()
    return _cache[name]


# ---- scalars ----------------------------------------------------------------------------------------------------------------------
def teeth_signs(k, teeth):
    """the sign bits of sc_teeth_signs: bit i set <=> s_i = +1, for the odd multiplier k or k + l"""
    cols = {5: 51, 6: 43, 7: 37}[teeth]
    k_odd = k if k & 1 else k + L
    return (k_odd >> 1) | (1 << (teeth * cols - 1)), cols


def column_negations(k, teeth=5):
    """per column, from the highest down: is the column's entry subtracted (what sc_teeth_next returns as `neg`)"""
    sg, cols = teeth_signs(k, teeth)
    return [not (sg >> (cols * (teeth - 1) + c)) & 1 for c in range(cols - 1, -1, -1)]


M55, MAA = int("55" * 32, 16) % 2**252, int("AA" * 32, 16) % 2**252      # the patterns 0x55..5 / 0xAA..A cut to canonical scalars


def comb_scalars():
    """[(name, k)]: the multipliers of the comb product.  The sign of a column is that of its top tooth.  In the 5 x 51 shape the top
    column is always added and, the odd multiplier being below 2^254, the one below it always subtracted; "all column signs equal" is
    therefore every column under the top one subtracted (odd multipliers below 2^205: no negation of the accumulator after the first),
    and the 0x55.. / 0xAA.. patterns flip the sign in every column they reach."""
    rng = random.Random("dbl-chain-scalars")
    out = [("0", 0), ("1", 1), ("2", 2), ("l-1", L - 1), ("l-2", L - 2), ("2^252", 2**252), ("2^253-1", 2**253 - 1),
           ("0x55", M55), ("0xAA", MAA), ("0x55 even", M55 - 1), ("0xAA odd", MAA | 1)]
    out += [("equal signs", 3), ("equal signs", 2**200 + 1), ("equal signs", 2**204 - 1), ("equal signs", 2**205 - 1)]
    for _ in range(6):                                  # even / odd pairs: the even one takes the k + l path
        k = rng.randrange(L) & ~1
        out += [("even", k), ("odd", k + 1)]
    out += [("random", rng.randrange(L)) for _ in range(200)]
    return out


def comb_digits(k, bits=20):
    """the signed digits of sc_comb_digit, lowest window first"""
    out, carry = [], 0
    for w in range(-(-254 // bits)):
        raw = ((k >> (bits * w)) & ((1 << bits) - 1)) + carry
        carry = (raw + (1 << (bits - 1))) >> bits
        out.append(raw - (carry << bits))
    assert carry == 0 and sum(d << (bits * w) for w, d in enumerate(out)) == k
    return out


def fixed_scalars(bits=20):
    """[(name, k)]: multipliers of the fixed comb with a zero digit in the first, a middle and the last window, and in every window"""
    rng = random.Random("dbl-chain-fixed")
    windows = -(-254 // bits)
    full = rng.randrange(2**253) | sum(1 << (bits * w) for w in range(windows - 1))     # no zero digit by itself
    # window w zero, and no carry into it: the top bit of the window below is cleared too
    clear = lambda k, w: k & ~(((1 << bits) - 1) << (bits * w)) & ~((1 << (bits * w - 1)) if w else 0)
    out = [("every window", 0), ("first", clear(full, 0)), ("middle", clear(full, windows // 2)), ("last", clear(full, windows - 1)),
           ("first and last", clear(clear(full, 0), windows - 1)), ("none", full)]
    # a digit that becomes zero through the carry of the window below it: window w all ones, window w - 1 at least 2^(bits - 1)
    w = 3
    out.append(("zero by carry", clear(full, w) | (((1 << bits) - 1) << (bits * w)) | (1 << (bits * w - 1))))
    out += [("random", rng.randrange(L)) for _ in range(20)]
    return out


def scalar_bytes(ks):
    return b"".join(k.to_bytes(32, "little") for k in ks)
