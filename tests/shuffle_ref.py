"""Model of the shuffle verifier (eg_shuffle_*; include/eg_hip.h, "re-encryption shuffles" has the rule): the Terelius-Wikstrom proof of a
re-encryption shuffle as restated by Haenni, Locher, Koenig and Dubuis, additively over Ristretto255 in the library's wire forms.  It holds
the rule (derive_key, verify) and a prover (shuffle, prove) for the tests and the probe.  Hashing is hashlib, scalars are Python integers,
and every point operation goes through a small backend of BATCHED primitives with two implementations:
  OracleBackend   the C restatement of the reference under oracle/ - the judge of the CPU tests and of the GPU tests' expectations
  LibraryBackend  the library's primitive tier (eg_mul_generator_batch, eg_vartime_double_mul_generator_batch, eg_vartime_multi_mul_batch):
                  the maker of large shuffles on a GPU box; never the judge.
The chain of the prover is built in its discrete-log form c^_i = [a_i]G + [b_i]H_0, so every prover step is one batched call."""
import hashlib
import random
import struct

L = (1 << 252) + 27742317777372353535851937790883648493
BAD_ENCODING, T1, T2, T3, T41, T42, CHAIN = 1, 2, 4, 8, 16, 32, 64
ROW_BAD, ROW_CHAIN = 1, 2
NONE = 0xFFFFFFFF
ROWS_MAX = 1 << 23
KEY_TRIES = 4096
HEAD = 288
IDENTITY = bytes(32)


def H32(x: bytes) -> bytes:
    return hashlib.sha512(x).digest()[:32]


def wide(x: bytes) -> int:
    return int.from_bytes(hashlib.sha512(x).digest(), "little") % L


def sc(k: int) -> bytes:
    return (k % L).to_bytes(32, "little")


def le64(i: int) -> bytes:
    return struct.pack("<Q", i)


def proof_bytes(n: int) -> int:
    return HEAD + 160 * n


def mth(leaves) -> bytes:
    """RFC 6962 2.1 over 32-byte leaf hashes, bottom up (the receipt log's tree; tests/merkle_ref.py has the recursion)"""
    if not leaves:
        return H32(b"")
    a = list(leaves)
    while len(a) > 1:
        a = [H32(b"\x01" + a[2 * i] + a[2 * i + 1]) if 2 * i + 1 < len(a) else a[2 * i] for i in range((len(a) + 1) // 2)]
    return a[0]


# ---------------------------------------------------------------------------------------------------------------- backends
class OracleBackend:
    """one oracle call per problem"""

    def __init__(self):
        from oracle import oracle as o

        self.o = o
        self.G = o.point_mul_generator(sc(1))

    def decodes(self, points):
        return [self.o.point_roundtrip(p) is not None for p in points]

    def mul_generator(self, ks):
        return [self.o.point_mul_generator(sc(k)) for k in ks]

    def double_mul_generator(self, ks, ps, rs):
        """[k]P + [r]G per problem; None where P does not decode"""
        return [self.o.point_double_mul_generator(sc(k), p, sc(r)) for k, p, r in zip(ks, ps, rs)]

    def multi_mul(self, terms, scalars, points):
        """len(scalars) / terms problems of `terms` terms; None where a point does not decode"""
        out = []
        for i in range(0, len(scalars), terms):
            out.append(self.o.point_multi_mul(b"".join(sc(k) for k in scalars[i:i + terms]), b"".join(points[i:i + terms])))
        return out

    def point_add(self, a, b, sub=False):
        return [self.o.point_add(x, y, sub) for x, y in zip(a, b)]


class LibraryBackend:
    """the library's primitive tier: one GPU call per step"""

    def __init__(self, ctx):
        import elastic_elgamal_amd as eg

        self.r = eg.Ristretto(ctx)
        self.G = self.r.mul_generator(sc(1))

    @staticmethod
    def _split(raw, ok=None):
        return [raw[32 * i:32 * i + 32] if ok is None or ok[i] else None for i in range(len(raw) // 32)]

    def decodes(self, points):
        if not points:
            return []
        return [bool(b) for b in self.r.element_roundtrip(b"".join(points))[1]]

    def mul_generator(self, ks):
        return self._split(self.r.mul_generator(b"".join(sc(k) for k in ks))) if ks else []

    def double_mul_generator(self, ks, ps, rs):
        if not ks:
            return []
        return self._split(*self.r.vartime_double_mul_generator(b"".join(sc(k) for k in ks), b"".join(ps), b"".join(sc(r) for r in rs)))

    def multi_mul(self, terms, scalars, points):
        if not scalars:
            return []
        return self._split(*self.r.vartime_multi_mul(terms, b"".join(sc(k) for k in scalars), b"".join(points)))

    def point_add(self, a, b, sub=False):
        if not a:
            return []
        return self._split(*self.r.element_add(b"".join(a), b"".join(b), sub))


# ---------------------------------------------------------------------------------------------------------------- the rule
def key_candidate(seed: bytes, j: int, ctr: int) -> bytes:
    d = bytearray(hashlib.sha512(b"eg-shuffle-v1/generator" + bytes([len(seed)]) + seed + le64(j) + struct.pack("<I", ctr)).digest()[:32])
    d[31] &= 0x7F
    return bytes(d)


def derive_key(be, seed: bytes, cap: int, tries: int = KEY_TRIES, with_tries: bool = False):
    """H_0 .. H_cap (cap + 1 elements): try-and-increment over the decoder, the smallest ctr that gives a non-identity element.
    Raises ValueError when a lane exhausts `tries`."""
    assert len(seed) <= 255
    key, used = [None] * (cap + 1), [0] * (cap + 1)
    todo, ctr = list(range(cap + 1)), 0
    while todo:
        if ctr >= tries:
            raise ValueError(f"generator {todo[0]}: no element in {tries} tries")
        cand = [key_candidate(seed, j, ctr) for j in todo]
        ok = be.decodes(cand)
        rest = []
        for j, c, good in zip(todo, cand, ok):
            if good and c != IDENTITY:
                key[j], used[j] = c, ctr + 1
            else:
                rest.append(j)
        todo, ctr = rest, ctr + 1
    return (key, used) if with_tries else key


def split_proof(n: int, proof: bytes):
    if len(proof) != proof_bytes(n):
        raise ValueError(f"a proof of {n} rows has {proof_bytes(n)} bytes, not {len(proof)}")
    head = [proof[32 * k:32 * k + 32] for k in range(9)]
    arr = [[proof[HEAD + (a * n + i) * 32:HEAD + (a * n + i) * 32 + 32] for i in range(n)] for a in range(5)]
    return head[:5], [int.from_bytes(s, "little") for s in head[5:]], arr       # t[5], s[4], (c, chat, that, shat, sprime)


def challenges_u(n, ins, outs, K, key, prefix, c):
    leaf1 = [H32(b"\x00" + ins[i] + outs[i] + c[i] + key[i + 1]) for i in range(n)]
    seed1 = hashlib.sha512(b"eg-shuffle-v1/seed" + bytes([len(prefix)]) + prefix + le64(n) + K + key[0] + mth(leaf1)).digest()
    return seed1, [wide(b"eg-shuffle-v1/u" + seed1 + le64(i)) for i in range(n)]


def challenge_x(n, seed1, chat, that, t):
    root2 = mth([H32(b"\x00" + chat[i] + that[i]) for i in range(n)])
    return wide(b"eg-shuffle-v1/c" + seed1 + root2 + b"".join(t))


def found_of(rows):
    f = [0, 0, NONE, NONE]
    for i, r in enumerate(rows):
        for b in (0, 1):
            if r >> b & 1:
                f[b] += 1
                f[2 + b] = min(f[2 + b], i)
    return f


def verify(be, ins, outs, K: bytes, key, prefix: bytes, proof: bytes):
    """(verdict mask, rows, found).  ins / outs: lists of 64-byte rows R || B; key: H_0 .. H_cap with cap >= N."""
    n = len(ins)
    if len(outs) != n or n > ROWS_MAX or len(key) < n + 1 or len(prefix) > 255:
        raise ValueError("bad statement")
    if n == 0:
        return 0, [], [0, 0, NONE, NONE]
    t, s, (c, chat, that, shat_b, sprime_b) = split_proof(n, proof)
    shat = [int.from_bytes(b, "little") for b in shat_b]
    sprime = [int.from_bytes(b, "little") for b in sprime_b]
    R, B = [r[:32] for r in ins], [r[32:] for r in ins]
    R2, B2 = [r[:32] for r in outs], [r[32:] for r in outs]
    dec = be.decodes(R + B + R2 + B2 + c + chat + list(key[:n + 1]) + [K])
    okR, okB, okR2, okB2, okc, okchat = (dec[k * n:(k + 1) * n] for k in range(6))
    rows = [0 if (okR[i] and okB[i] and okR2[i] and okB2[i] and okc[i] and okchat[i] and shat[i] < L and sprime[i] < L) else ROW_BAD for i in range(n)]
    bad = any(rows) or not all(dec[6 * n:]) or any(v >= L for v in s)
    seed1, u = challenges_u(n, ins, outs, K, key, prefix, c)
    x = challenge_x(n, seed1, chat, that, t)
    # CHAIN, row by row: evaluated where both chain elements decode and both scalars are canonical
    prev = [key[0]] + chat[:-1]
    okprev = [dec[6 * n]] + okchat[:-1]
    ev = [i for i in range(n) if okchat[i] and okprev[i] and shat[i] < L and sprime[i] < L]
    sc3, pt3 = [], []
    for i in ev:
        sc3 += [-x, sprime[i], shat[i]]
        pt3 += [chat[i], prev[i], be.G]
    for i, got in zip(ev, be.multi_mul(3, sc3, pt3)):
        if got != that[i]:
            rows[i] |= ROW_CHAIN
    found = found_of(rows)
    if bad:
        return BAD_ENCODING, rows, found
    mask = CHAIN if found[1] else 0
    xu = [-x * ui for ui in u]
    uprod = 1
    for ui in u:
        uprod = uprod * ui % L
    H = list(key[1:n + 1])
    G = be.G
    rhs = be.multi_mul(2 * n + 1, [-x] * n + [x] * n + [s[0]] + xu + sprime + [s[2]] + xu + sprime + [-s[3]] + xu + sprime + [-s[3]],
                       c + H + [G] + c + H + [G] + B + B2 + [K] + R + R2 + [G])
    rhs2 = be.multi_mul(3, [-x, x * uprod, s[1]], [chat[n - 1], key[0], G])[0]
    for bit, got, want in ((T1, rhs[0], t[0]), (T2, rhs2, t[1]), (T3, rhs[1], t[2]), (T41, rhs[2], t[3]), (T42, rhs[3], t[4])):
        if got != want:
            mask |= bit
    return mask, rows, found


# ---------------------------------------------------------------------------------------------------------------- the prover
def encrypt(be, K: bytes, msgs, rs):
    """rows R || B = [r]G || [m]G + [r]K"""
    R = be.mul_generator(rs)
    B = be.double_mul_generator(rs, [K] * len(rs), msgs)
    return [a + b for a, b in zip(R, B)]


def shuffle(be, ins, K: bytes, src, rho):
    """out_i = in_src[i] + ([rho_i]G, [rho_i]K)"""
    n = len(ins)
    R2 = be.double_mul_generator([1] * n, [ins[src[i]][:32] for i in range(n)], rho)
    B2 = be.multi_mul(2, [v for i in range(n) for v in (1, rho[i])], [p for i in range(n) for p in (ins[src[i]][32:], K)])
    return [a + b for a, b in zip(R2, B2)]


def prove(be, ins, outs, K: bytes, key, prefix: bytes, src, rho, rng: random.Random, pi=None, that_flip=None):
    """The honest prover on the statement (ins, outs) with the witness (src, rho).  `pi` (row j of c commits to H_{pi[j] + 1}) defaults to the
    inverse of src; a lying prover hands in a pi that is no permutation, or outs that are no shuffle of ins, or (that_flip = k)
    commits to a t^_k with one bit flipped and answers the challenge that follows from it."""
    n = len(ins)
    rnd = lambda: rng.getrandbits(512) % L
    if pi is None:
        pi = [0] * n
        for i in range(n):
            pi[src[i]] = i
    r = [rnd() for _ in range(n)]
    c = be.double_mul_generator([1] * n, [key[pi[j] + 1] for j in range(n)], r)
    seed1, u = challenges_u(n, ins, outs, K, key, prefix, c)
    up = [u[src[i]] for i in range(n)]
    rhat = [rnd() for _ in range(n)]
    a, b, ai, bi = [], [], 0, 1
    for i in range(n):
        ai, bi = (rhat[i] + up[i] * ai) % L, up[i] * bi % L
        a.append(ai)
        b.append(bi)
    chat = be.double_mul_generator(b, [key[0]] * n, a)
    w1, w2, w3, w4 = rnd(), rnd(), rnd(), rnd()
    what, wp = [rnd() for _ in range(n)], [rnd() for _ in range(n)]
    R2, B2 = [o[:32] for o in outs], [o[32:] for o in outs]
    t1, t2 = be.mul_generator([w1, w2])
    t3, t41, t42 = be.multi_mul(n + 1, wp + [w3] + wp + [-w4] + wp + [-w4], list(key[1:n + 1]) + [be.G] + B2 + [K] + R2 + [be.G])
    that = be.double_mul_generator(wp, [key[0]] + chat[:-1], what)
    t = [t1, t2, t3, t41, t42]
    if that_flip is not None:
        that[that_flip] = bytes([that[that_flip][0], that[that_flip][1] ^ 4]) + that[that_flip][2:]
    x = challenge_x(n, seed1, chat, that, t)
    s = [w1 + x * sum(r), w2 + x * a[-1], w3 + x * sum(rj * uj for rj, uj in zip(r, u)), w4 + x * sum(p * q for p, q in zip(rho, up))]
    shat = [what[i] + x * rhat[i] for i in range(n)]
    sprime = [wp[i] + x * up[i] for i in range(n)]
    return b"".join(t) + b"".join(sc(v) for v in s) + b"".join(c) + b"".join(chat) + b"".join(that) + b"".join(sc(v) for v in shat) + \
        b"".join(sc(v) for v in sprime)


def make(be, K: bytes, key, prefix: bytes, n: int, seed: int, perm: str = "random"):
    """an honest case: dict(ins, outs, proof, src, rho, msgs) - plaintexts 1 .. n, everything else from random.Random(seed)"""
    rng = random.Random(seed)
    msgs = list(range(1, n + 1))
    ins = encrypt(be, K, msgs, [rng.getrandbits(512) % L for _ in range(n)])
    src = list(range(n))
    if perm == "random":
        rng.shuffle(src)
    elif perm == "reverse":
        src.reverse()
    rho = [rng.getrandbits(512) % L for _ in range(n)]
    outs = shuffle(be, ins, K, src, rho)
    return {"ins": ins, "outs": outs, "src": src, "rho": rho, "msgs": msgs, "proof": prove(be, ins, outs, K, key, prefix, src, rho, rng)}
