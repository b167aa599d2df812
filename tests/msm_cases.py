"""Multi-scalar products at the sizes where the bucket method runs (test infrastructure; no GPU).

The primitive tier's Group::vartime_multi_mul switches from Straus to the bucket method (elastic_elgamal_amd/csrc/pippenger.cuh) at 2^20
terms per problem and accepts up to 2^24.  The oracle's point_multi_mul does a scalar multiplication per term on one CPU thread, so it
cannot follow those sizes.  An exact reference needs no multi-scalar product at all when every point has a known discrete log:

    P_t = [x_t]G   =>   sum_t [k_t]P_t + [r]G = [(sum_t k_t x_t + r) mod l]G

The sum is exact integer arithmetic, and the expected encoding costs one oracle.point_mul_generator.  Points come from a Pool of known
logs; a term names its point by index, so sum_t k_t x_t = sum_j x_j K_j with K_j the sum of the scalars of the terms that use point j.

The module also restates what the bucket method does with a case (the window width, the level count, the signed recoding of
k_pip_prepare), so that the CPU tests can assert that every GPU case reaches the edge it is named for.  MATRIX lists the GPU cases.
"""
from __future__ import annotations

import random
from dataclasses import dataclass

import numpy as np

from oracle import oracle as o

L = o.L
IDENTITY = bytes(32)
UNDECODABLE = b"\xff" * 32              # not a canonical field element: does not decode
MAX_TERMS = 1 << 24                     # include/eg_hip.h: at most 2^24 terms per problem
POOL_SIZE = 1 << 16


def sc(x: int) -> bytes:
    return (x % L).to_bytes(32, "little")


# ---- model of the bucket method (eg_hip.hip: pip_window_bits, pip_layout; pippenger.cuh: pip_windows, k_pip_prepare) ----------------
PIP_MIN_C, PIP_MAX_C, PIP_S_TERMS, PIP_S_POINTS = 12, 15, 128, 64


def window_bits(terms: int) -> int:
    c = PIP_MIN_C
    while c < PIP_MAX_C and (64 << (c - 1)) < terms:
        c += 1
    return c


def windows(c: int) -> int:
    return (256 + c) // c


def levels(terms: int) -> int:
    lv, n = 1, -(-terms // PIP_S_TERMS)
    while n > 1:
        n = -(-n // PIP_S_POINTS)
        lv += 1
    return lv


def layout(terms: int) -> dict:
    """c, W, the level count and the number of 1024-bucket tiles of k_pip_scan_* for one problem of `terms` terms."""
    c = window_bits(terms)
    return {"c": c, "W": windows(c), "levels": levels(terms), "tiles": -(-windows(c) * (1 << (c - 1)) // 1024)}


def recode(scalars: np.ndarray, c: int):
    """k_pip_prepare's signed c-bit recoding of (n, 32) little-endian scalars: (digits, carries), both (W, n).  Window w reads the 64
    bits of words wi, wi + 1 from bit c w, adds the carry of the window below, and a raw value above 2^(c-1) becomes the negative digit
    raw - 2^c with a carry into the next window.  k = sum_w digits[w] 2^(c w) for every k < 2^256 - 2^(c W - 1)."""
    n = len(scalars)
    words = np.zeros((n, 9), np.uint64)
    words[:, :8] = np.ascontiguousarray(scalars).view("<u4")
    W, B, mask = windows(c), 1 << (c - 1), np.uint64((1 << c) - 1)
    digits, carries = np.zeros((W, n), np.int32), np.zeros((W, n), bool)
    carry = np.zeros(n, np.uint64)
    for w in range(W):
        wi, sh = (w * c) >> 5, np.uint64((w * c) & 31)
        v = words[:, wi] | (words[:, wi + 1] << np.uint64(32))
        raw = ((v >> sh) & mask) + carry
        carries[w] = raw > B
        carry = carries[w].astype(np.uint64)
        digits[w] = np.where(carries[w], raw.astype(np.int64) - (1 << c), raw.astype(np.int64))
    return digits, carries


def bucket_stats(scalars: np.ndarray, c: int) -> dict:
    """What a problem with these scalars reaches in the bucket method at window width c: the longest bucket, whether a non-empty bucket
    has index >= 2^13 (k_pip_window: bit 13 of the segment weight b0), the number of empty buckets and the longest carry chain."""
    digits, carries = recode(scalars, c)
    B = 1 << (c - 1)
    counts = np.stack([np.bincount(np.abs(d[d != 0]) - 1, minlength=B) for d in digits])
    run = longest = np.zeros(len(scalars), np.int64)
    for cw in carries:
        run = (run + 1) * cw
        longest = np.maximum(longest, run)
    return {"max_bucket": int(counts.max()), "high_bucket": bool(counts[:, 1 << 13:].any()), "empty": int((counts == 0).sum()),
            "carry_chain": int(longest.max()) if len(scalars) else 0}


# ---- points of known log and the exact reference ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Pool:
    """Logs of the points the cases use.  Entry half + j is the negative of entry j, for the cancelling pairs; entries 0 and half are
    the identity, 1 is G and half + 1 is -G, 2 is [2]G."""
    logs: tuple

    def __len__(self):
        return len(self.logs)

    @property
    def half(self) -> int:
        return len(self.logs) // 2

    def encoding(self, j: int) -> bytes:
        return o.point_mul_generator(sc(self.logs[j]))


def make_pool(size: int = POOL_SIZE, seed: int = 4096) -> Pool:
    rnd = random.Random(seed)
    base = [0, 1, 2] + [rnd.randrange(1, L) for _ in range(size // 2 - 3)]
    return Pool(tuple(base + [(L - x) % L for x in base]))


def exact_log(scalars: np.ndarray, idx: np.ndarray, pool: Pool) -> int:
    """(sum_t k_t x_idx[t]) mod l, exactly.  K_j is summed in 16-bit limbs with bincount, which returns float64: a bin holds at most
    2^24 limbs below 2^16, so every partial sum is below 2^40 < 2^53 and no bit is lost."""
    n = len(idx)
    assert n <= MAX_TERMS and scalars.shape == (n, 32) and scalars.dtype == np.uint8
    limbs = np.ascontiguousarray(scalars).view("<u2")
    total = 0
    for i in range(16):
        s = np.bincount(idx, weights=limbs[:, i], minlength=len(pool))
        assert s.max(initial=0) < 2.0**53
        total += sum(int(v) * x for v, x in zip(s.tolist(), pool.logs) if v) << (16 * i)
    return total % L


@dataclass
class Case:
    """One problem: scalars (n, 32) uint8, all canonical; idx (n,) pool indices; r the generator term of the device entries; bad the
    term indices whose encoding is replaced by an undecodable one (the problem is flagged and such a term contributes nothing)."""
    scalars: np.ndarray
    idx: np.ndarray
    r: int = 0
    bad: tuple = ()

    @property
    def terms(self) -> int:
        return len(self.idx)

    def log(self, pool: Pool, with_r: bool = False) -> int:
        s = self.scalars
        if self.bad:
            s = s.copy()
            s[list(self.bad)] = 0
        return (exact_log(s, self.idx, pool) + (self.r if with_r else 0)) % L

    def expected(self, pool: Pool, with_r: bool = False) -> bytes:
        return o.point_mul_generator(sc(self.log(pool, with_r)))

    def scalar_ints(self):
        return [int.from_bytes(bytes(row), "little") for row in self.scalars]


def _from_ints(values) -> np.ndarray:
    return np.frombuffer(b"".join(sc(v) for v in values), np.uint8).reshape(-1, 32).copy()


def random_scalars(rng: np.random.Generator, n: int) -> np.ndarray:
    s = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    s[:, 31] &= 0x0F                       # below 2^252 < l
    if n:
        s[0] = _from_ints([L - 1])[0]
    return s


def digit_patterns(c: int) -> list:
    """Scalars whose c-bit windows hold given raw digits (B = 2^(c-1)): B in every window (the top bucket), B + 1 (a negative digit and
    a carry out of every window), 2^c - 1 (digit -1, then 0 with a carry running through every window), and one non-zero window at
    each position in turn.  The windows above bit 251 are clipped so that the scalar stays below l; l - 1 is added."""
    B, W, clip = 1 << (c - 1), windows(c), (1 << 252) - 1
    every = [sum(d << (c * w) for w in range(W)) & clip for d in (B, B + 1, (1 << c) - 1)]
    single = [(d << (c * w)) & clip for w in range(W) for d in (1, B, B + 1, (1 << c) - 1)]
    out = []
    for v in every + single + [L - 1]:
        if v and v not in out:
            out.append(v)
    return out


def build(mode: str, terms: int, pool: Pool, seed: int) -> list:
    """The problems of one case (two for mode "two", one otherwise).  Modes: random, equal, digits, sparse, zero, pairs, cancel, bad."""
    rng = np.random.default_rng(seed)
    r = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % L
    idx = rng.integers(0, len(pool), terms, dtype=np.int64)
    if mode == "random":
        return [Case(random_scalars(rng, terms), idx, r)]
    if mode == "equal":                    # one scalar for every term: each window has one bucket that holds every term
        k = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % L
        return [Case(np.repeat(_from_ints([k]), terms, axis=0), idx, r)]
    if mode == "digits":
        pats = _from_ints(digit_patterns(window_bits(terms)))
        return [Case(pats[np.arange(terms) % len(pats)], idx, r)]
    if mode == "sparse":                   # 99.9 % zero scalars: long runs of empty buckets
        s = random_scalars(rng, terms)
        s[rng.random(terms) >= 0.001] = 0
        return [Case(s, idx, r)]
    if mode == "zero":
        return [Case(np.zeros((terms, 32), np.uint8), idx, r)]
    if mode == "pairs":                    # x and l - x with equal scalars: every bucket sums to the identity
        h = pool.half
        j = rng.integers(0, h, (terms + 1) // 2, dtype=np.int64)
        pidx = np.stack([j, j + h], axis=1).reshape(-1)[:terms]
        s = np.repeat(random_scalars(rng, (terms + 1) // 2), 2, axis=0)[:terms].copy()
        if terms % 2:
            s[-1] = 0
        return [Case(s, pidx, r)]
    if mode == "cancel":                   # the last scalar makes the total 0 mod l
        s = random_scalars(rng, terms)
        idx[-1] = 3
        s[-1] = 0
        rest = exact_log(s, idx, pool)
        s[-1] = _from_ints([-rest * pow(pool.logs[3], -1, L)])[0]
        return [Case(s, idx, r)]
    if mode == "bad":                      # identities mixed in; undecodable encodings at the first and the last term
        idx[::16] = 0
        idx[5::16] = pool.half
        return [Case(random_scalars(rng, terms), idx, r, bad=(0, terms - 1))]
    if mode == "two":                      # two problems, different operands, over one scratch buffer
        return build("equal", terms, pool, seed + 1) + build("random", terms, pool, seed + 2)
    raise ValueError(mode)


MODES = ("random", "equal", "digits", "sparse", "zero", "pairs", "cancel", "bad", "two")


# ---- the GPU matrix -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Spec:
    """One GPU case.  ctx: "forced" (EG_MSM_BUCKET_MIN=4096) or "default" (the shipped switch at 2^20 terms); entries: "host"
    (eg_vartime_multi_mul_batch), "device" (with d_r and d_ok), "prepared" (over prepared points, with d_r); needs: what the model must
    show the case reaches (layout keys c, levels, tiles; data keys min_bucket, high_bucket, min_carry_chain, min_empty; log_zero)."""
    name: str
    ctx: str
    terms: int
    mode: str
    entries: tuple
    needs: tuple
    seed: int = 1

    @property
    def need(self) -> dict:
        return dict(self.needs)


_ALL = ("host", "device", "prepared")
_C15 = (("c", 15), ("levels", 4), ("tiles", 288))
MATRIX = (
    Spec("c12_random", "forced", 1 << 17, "random", ("device",), (("c", 12), ("levels", 3), ("tiles", 44)), 11),
    Spec("c13_random", "forced", (1 << 17) + 1, "random", ("device",), (("c", 13), ("tiles", 80)), 12),
    Spec("c13_digits", "forced", (1 << 17) + 1, "digits", ("device",), (("c", 13), ("tiles", 80), ("min_carry_chain", 19)), 13),
    Spec("c14_random", "forced", (1 << 18) + 1, "random", ("device",), (("c", 14), ("tiles", 152)), 14),
    Spec("c14_digits", "forced", (1 << 18) + 1, "digits", ("device",), (("c", 14), ("tiles", 152), ("min_carry_chain", 18)), 15),
    Spec("c15_random", "forced", (1 << 19) + 1, "random", _ALL, _C15 + (("high_bucket", True),), 16),
    Spec("c15_equal", "forced", (1 << 19) + 1, "equal", _ALL, _C15 + (("high_bucket", True), ("min_bucket", 128 * 64 * 64 + 1)), 17),
    Spec("c15_digits", "forced", (1 << 19) + 1, "digits", ("device",), _C15 + (("high_bucket", True), ("min_carry_chain", 16)), 18),
    Spec("c15_sparse", "forced", (1 << 19) + 1, "sparse", ("device",), _C15 + (("high_bucket", True), ("min_empty", 18 * (16384 - 1024))), 19),
    Spec("c15_zero", "forced", (1 << 19) + 1, "zero", ("host", "device"), _C15 + (("min_empty", 18 * 16384), ("log_zero", True)), 20),
    Spec("c15_pairs", "forced", (1 << 19) + 1, "pairs", ("host", "device"), _C15 + (("high_bucket", True), ("log_zero", True)), 21),
    Spec("c15_cancel", "forced", (1 << 19) + 1, "cancel", ("host", "device"), _C15 + (("high_bucket", True), ("log_zero", True)), 22),
    Spec("c15_bad", "forced", (1 << 19) + 1, "bad", ("host", "device"), _C15 + (("high_bucket", True),), 23),
    Spec("c15_two", "forced", (1 << 19) + 1, "two", ("host", "device"), _C15 + (("high_bucket", True), ("min_bucket", 128 * 64 * 64 + 1)), 24),
    Spec("straus_last", "default", (1 << 20) - 1, "random", ("device",), (("buckets", False),), 25),
    Spec("bucket_first", "default", 1 << 20, "random", ("device", "prepared"), _C15 + (("buckets", True), ("high_bucket", True)), 26),
    Spec("bucket_ragged", "default", (1 << 20) + 255, "random", ("device",), _C15 + (("buckets", True), ("high_bucket", True)), 27),
    Spec("advertised", "default", 1 << 22, "random", ("device", "prepared"), _C15 + (("buckets", True),), 28),
    Spec("maximum", "default", 1 << 24, "random", ("device",), _C15 + (("buckets", True),), 29),
)
DATA_KEYS = ("high_bucket", "min_bucket", "min_carry_chain", "min_empty", "log_zero")
DEFAULT_BUCKET_MIN, FORCED_BUCKET_MIN = 1 << 20, 4096


def uses_buckets(spec: Spec) -> bool:
    return spec.terms >= (FORCED_BUCKET_MIN if spec.ctx == "forced" else DEFAULT_BUCKET_MIN)
