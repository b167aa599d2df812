"""ristretto255 on Python integers: extended twisted-Edwards points (X : Y : Z : T) on -x^2 + y^2 = 1 + d x^2 y^2, the
decoding and encoding of RFC 9496 section 4.3, double-and-add products.

An element of the group is a coset of E[4]; equality and serialisation go through `encode`, as in the reference
(`serialize_element`, src/group/ristretto.rs:88-90)."""
from .field import D, INVSQRT_A_MINUS_D, L, P, SQRT_M1, ct_abs, inv, is_negative, sqrt_ratio_m1

IDENTITY = (0, 1, 1, 0)
D2 = 2 * D % P


def _basepoint():
    """The Ed25519 basepoint: y = 4/5, x the non-negative root of (y^2 - 1) / (d y^2 + 1)."""
    y = 4 * inv(5) % P
    ok, x = sqrt_ratio_m1(y * y - 1, D * y * y + 1)
    assert ok
    return (x, y, 1, x * y % P)


BASEPOINT = _basepoint()
# E[4], the coset of the identity: (0, 1), (0, -1), (i, 0), (-i, 0)
TORSION4 = ((0, 1, 1, 0), (0, P - 1, 1, 0), (SQRT_M1, 0, 1, 0), (P - SQRT_M1, 0, 1, 0))


def on_curve(pt) -> bool:
    x, y, z, t = pt
    return (-x * x + y * y - z * z - D * t * t) % P == 0 and (x * y - z * t) % P == 0


def add(p1, p2):
    """The unified addition law for a = -1 (Hisil, Wong, Carter, Dawson 2008, section 3.1); complete because d is no square."""
    x1, y1, z1, t1 = p1
    x2, y2, z2, t2 = p2
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = t1 * D2 % P * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def double(p1):
    x1, y1, z1, _ = p1
    a = x1 * x1 % P
    b = y1 * y1 % P
    c = 2 * z1 * z1 % P
    e = ((x1 + y1) * (x1 + y1) - a - b) % P
    g = b - a
    f = g - c
    h = -a - b
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def neg(p1):
    x, y, z, t = p1
    return ((-x) % P, y, z, (-t) % P)


def sub(p1, p2):
    return add(p1, neg(p2))


def mul(k: int, pt):
    """[k]P by double-and-add from the top bit; k is taken as given (not reduced)."""
    assert k >= 0
    acc = IDENTITY
    for i in range(k.bit_length() - 1, -1, -1):
        acc = double(acc)
        if (k >> i) & 1:
            acc = add(acc, pt)
    return acc


def multi_mul(scalars, points):
    """sum [k_i]P_i with one shared chain of doublings (vartime_multi_mul, src/group/ristretto.rs:139-145)."""
    scalars, points = list(scalars), list(points)
    assert len(scalars) == len(points)
    acc = IDENTITY
    top = max((k.bit_length() for k in scalars), default=0)
    for i in range(top - 1, -1, -1):
        acc = double(acc)
        for k, pt in zip(scalars, points):
            if (k >> i) & 1:
                acc = add(acc, pt)
    return acc


def mul_generator(k: int):
    return mul(k, BASEPOINT)


def double_mul_generator(k: int, pt, r: int):
    """[k]P + [r]G (vartime_double_mul_generator, src/group/ristretto.rs:131-137)."""
    return multi_mul((k, r), (pt, BASEPOINT))


def decode(b: bytes):
    """RFC 9496 4.3.1; None where CompressedRistretto::decompress returns None (src/group/ristretto.rs:93-95)."""
    assert len(b) == 32
    s = int.from_bytes(b, "little")
    if s >= P or s & 1:
        return None
    ss = s * s % P
    u1 = (1 - ss) % P
    u2 = (1 + ss) % P
    u2_sqr = u2 * u2 % P
    v = (-(D * u1 % P * u1) - u2_sqr) % P
    was_square, invsqrt = sqrt_ratio_m1(1, v * u2_sqr % P)
    den_x = invsqrt * u2 % P
    den_y = invsqrt * den_x % P * v % P
    x = ct_abs(2 * s * den_x % P)
    y = u1 * den_y % P
    t = x * y % P
    if not was_square or is_negative(t) or y == 0:
        return None
    return (x, y, 1, t)


def encode(pt) -> bytes:
    """RFC 9496 4.3.2."""
    x0, y0, z0, t0 = pt
    u1 = (z0 + y0) * (z0 - y0) % P
    u2 = x0 * y0 % P
    _, invsqrt = sqrt_ratio_m1(1, u1 * u2 % P * u2 % P)
    den1 = invsqrt * u1 % P
    den2 = invsqrt * u2 % P
    z_inv = den1 * den2 % P * t0 % P
    ix0 = x0 * SQRT_M1 % P
    iy0 = y0 * SQRT_M1 % P
    enchanted_denominator = den1 * INVSQRT_A_MINUS_D % P
    if is_negative(t0 * z_inv % P):
        x, y, den_inv = iy0, ix0, enchanted_denominator
    else:
        x, y, den_inv = x0, y0, den2
    if is_negative(x * z_inv % P):
        y = (-y) % P
    return ct_abs(den_inv * (z0 - y) % P).to_bytes(32, "little")


def equal(p1, p2) -> bool:
    """Equality of ristretto elements (RFC 9496 4.3.3): x1 y2 == y1 x2 or y1 y2 == x1 x2."""
    x1, y1, _, _ = p1
    x2, y2, _, _ = p2
    return (x1 * y2 - y1 * x2) % P == 0 or (y1 * y2 - x1 * x2) % P == 0


def is_identity(pt) -> bool:
    return equal(pt, IDENTITY)


assert on_curve(BASEPOINT) and all(on_curve(t) for t in TORSION4) and L > 0
