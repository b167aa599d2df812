"""RFC 8032 Ed25519 in Python integers (extended coordinates: a verification costs milliseconds), and the rule of the GPU pass
(include/eg_hip.h, "voter signatures") with its status words.  Needs nothing but hashlib.

verify_detail() is the rule in full; expected_status() is the cheap form for large batches: it needs no scalar multiplication for an
item the caller KNOWS to be tampered (S >= l is an integer compare, the key decode one modular power, a valid key with anything else
tampered is detail 4) - only an item that is claimed to be valid gets the full check."""
import hashlib

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)

ST_BAD_SIGNATURE = 15
BAD_S, BAD_KEY, SMALL_ORDER, MISMATCH, BAD_INDEX = 1, 2, 3, 4, 5


def status_word(detail: int) -> int:
    return 0 if detail == 0 else ST_BAD_SIGNATURE | (detail << 8)


def _recover_x(y: int, sign: int):
    """RFC 8032 5.1.3, strict: None when y >= p, when there is no square root, or when x = 0 carries the sign bit."""
    if y >= P:
        return None
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = (u * pow(v, 3, P) * pow(u * pow(v, 7, P) % P, (P - 5) // 8, P)) % P
    vxx = v * x * x % P
    if vxx == u:
        pass
    elif vxx == (-u) % P:
        x = x * SQRT_M1 % P
    else:
        return None
    if x == 0 and sign:
        return None
    if (x & 1) != sign:
        x = P - x
    return x


def decode(enc: bytes):
    """-> extended point (X, Y, Z, T) or None"""
    v = int.from_bytes(enc, "little")
    y, sign = v & ((1 << 255) - 1), v >> 255
    x = _recover_x(y, sign)
    return None if x is None else (x, y, 1, x * y % P)


def encode(p) -> bytes:
    zi = pow(p[2], P - 2, P)
    x, y = p[0] * zi % P, p[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def add(p, q):
    a = (p[1] - p[0]) * (q[1] - q[0]) % P
    b = (p[1] + p[0]) * (q[1] + q[0]) % P
    c = 2 * D * p[3] * q[3] % P
    d = 2 * p[2] * q[2] % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def neg(p):
    return ((-p[0]) % P, p[1], p[2], (-p[3]) % P)


IDENT = (0, 1, 1, 0)
_BY = 4 * pow(5, P - 2, P) % P
B = (_recover_x(_BY, 0), _BY, 1, _recover_x(_BY, 0) * _BY % P)


def mul(k: int, p):
    q = IDENT
    while k:
        if k & 1:
            q = add(q, p)
        p = add(p, p)
        k >>= 1
    return q


def is_identity(p) -> bool:
    return p[0] % P == 0 and (p[1] - p[2]) % P == 0


def is_small_order(p) -> bool:
    return is_identity(mul(8, p))


def _h(*parts) -> int:
    return int.from_bytes(hashlib.sha512(b"".join(parts)).digest(), "little")


def expand_seed(seed: bytes):
    d = hashlib.sha512(seed).digest()
    a = int.from_bytes(d[:32], "little")
    a = (a & ((1 << 254) - 8)) | (1 << 254)
    return a, d[32:]


def public_key(seed: bytes) -> bytes:
    return encode(mul(expand_seed(seed)[0], B))


def sign(seed: bytes, msg: bytes) -> bytes:
    a, hp = expand_seed(seed)
    A = encode(mul(a, B))
    r = _h(hp, msg) % L
    R = encode(mul(r, B))
    s = (r + (_h(R, A, msg) % L) * a) % L
    return R + s.to_bytes(32, "little")


def verify_detail(key: bytes, msg: bytes, sig: bytes) -> int:
    """The rule, checks 2..5 of the header (the roster index is the caller's): 0 = accepted, else the detail."""
    R, s = sig[:32], int.from_bytes(sig[32:], "little")
    if s >= L:
        return BAD_S
    A = decode(key)
    if A is None:
        return BAD_KEY
    if is_small_order(A):
        return SMALL_ORDER
    h = _h(R, key, msg) % L
    return 0 if encode(add(mul(s, B), mul(h, neg(A)))) == R else MISMATCH


def verify(key: bytes, msg: bytes, sig: bytes) -> bool:
    return verify_detail(key, msg, sig) == 0


_key_cache = {}


def key_detail(key: bytes) -> int:
    """0, BAD_KEY or SMALL_ORDER: what the key alone decides (cached: rosters repeat)."""
    d = _key_cache.get(key)
    if d is None:
        A = decode(key)
        d = BAD_KEY if A is None else SMALL_ORDER if is_small_order(A) else 0
        _key_cache[key] = d
    return d


def expected_status(key: bytes, msg: bytes, sig: bytes, tampered: bool, index_ok: bool = True) -> int:
    """Status word of the pass.  tampered=True: the caller broke a valid item (any bit of R, S, A, the message, the prefix, or the roster
    index), so the equation cannot hold and no scalar multiplication is needed.  tampered=False: the full check."""
    if not index_ok:
        return status_word(BAD_INDEX)
    if int.from_bytes(sig[32:], "little") >= L:
        return status_word(BAD_S)
    kd = key_detail(key)
    if kd:
        return status_word(kd)
    if tampered:
        return status_word(MISMATCH)
    return status_word(verify_detail(key, msg, sig))


def small_order_encodings():
    """The eight encodings of the points of order 1, 2, 4, 4, 8, 8, 8, 8 (canonical y, both signs where x != 0)."""
    out = []
    p8 = None
    y = 2
    while p8 is None:                      # a point whose multiple by l has order exactly 8
        for sgn in (0, 1):
            pt = decode((y | (sgn << 255)).to_bytes(32, "little"))
            if pt is not None:
                t = mul(L, pt)
                if not is_identity(mul(4, t)):
                    p8 = t
                    break
        y += 1
    q = IDENT
    for _ in range(8):
        out.append(encode(q))
        q = add(q, p8)
    assert len(set(out)) == 8 and is_identity(q)
    return out
