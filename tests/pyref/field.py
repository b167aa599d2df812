"""Arithmetic mod p = 2^255 - 19 and mod l (the order of the ristretto255 group) on Python integers; constants and
SQRT_RATIO_M1 of RFC 9496 section 4.1 / 4.2."""

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493

D = (-121665 * pow(121666, P - 2, P)) % P                # RFC 9496 4.1
SQRT_M1 = pow(2, (P - 1) // 4, P)                        # a square root of -1: 2 is a non-residue and p = 5 mod 8
assert SQRT_M1 * SQRT_M1 % P == P - 1


def inv(x: int) -> int:
    return pow(x, P - 2, P)


def is_negative(x: int) -> bool:
    """RFC 9496 4.2: the low bit of the canonical representative."""
    return (x % P) & 1 == 1


def ct_abs(x: int) -> int:
    x %= P
    return P - x if x & 1 else x


def sqrt_ratio_m1(u: int, v: int):
    """RFC 9496 4.2: (was_square, r) with r the non-negative square root of u / v, or of SQRT_M1 * u / v."""
    u %= P
    v %= P
    v3 = v * v % P * v % P
    v7 = v3 * v3 % P * v % P
    r = u * v3 % P * pow(u * v7 % P, (P - 5) // 8, P) % P
    check = v * r % P * r % P
    correct_sign = check == u
    flipped_sign = check == (-u) % P
    flipped_sign_i = check == (-u) * SQRT_M1 % P
    if flipped_sign or flipped_sign_i:
        r = r * SQRT_M1 % P
    return (correct_sign or flipped_sign), ct_abs(r)


# 1 / sqrt(a - d) with a = -1: the non-negative root (RFC 9496 4.1 lists the same number)
_ok, INVSQRT_A_MINUS_D = sqrt_ratio_m1(1, (-1 - D) % P)
assert _ok and INVSQRT_A_MINUS_D * INVSQRT_A_MINUS_D % P * ((-1 - D) % P) % P == 1


# ------------------------------------------------------------------ scalars
def scalar_from_canonical_bytes(b: bytes):
    """Scalar::from_canonical_bytes (src/group/ristretto.rs:59-62): None unless the 32 bytes are a number below l."""
    assert len(b) == 32
    s = int.from_bytes(b, "little")
    return s if s < L else None


def scalar_from_wide(b: bytes) -> int:
    """Scalar::from_bytes_mod_order_wide (src/group/ristretto.rs:34-38)."""
    assert len(b) == 64
    return int.from_bytes(b, "little") % L


def scalar_bytes(s: int) -> bytes:
    return (s % L).to_bytes(32, "little")
