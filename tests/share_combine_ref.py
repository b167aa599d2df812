"""Restatement of ``lagrange_coefficients`` and ``Params::combine_shares`` (src/sharing/mod.rs:139-170, 302-325) on the CPU oracle's
scalar functions and ``point_multi_mul``, with the selection rule of the batch entry (eg_combine_shares_batch) on top, and the Shamir
key sets and share items the tests of the batch entry use.  Nothing here calls the library under test."""
import random

L = 2**252 + 27742317777372353535851937790883648493
OK = 0
ZERO32 = bytes(32)


def sc(x: int) -> bytes:
    return (x % L).to_bytes(32, "little")


# ------------------------------------------------------------------ the reference's two functions
def lagrange_coefficients(oracle, indexes):
    """([1 / signed denominator_i], scale) for zero-based participant indexes: the points are index + 1"""
    denominators = []
    for index in indexes:
        sign, magnitude = False, sc(1)
        for other in indexes:
            if index > other:
                elem_sign, elem = True, sc(index - other)
            elif index < other:
                elem_sign, elem = False, sc(other - index)
            else:
                elem_sign, elem = False, sc(index + 1)
            sign, magnitude = sign ^ elem_sign, oracle.sc_mul(magnitude, elem)
        denominators.append(oracle.sc_neg(magnitude) if sign else magnitude)
    inverted = [oracle.sc_invert(d) for d in denominators]            # G::invert_scalars
    scale = sc(1)
    for index in indexes:
        scale = oracle.sc_mul(scale, sc(index + 1))
    return inverted, scale


def combine_shares(oracle, shares_n, threshold, given):
    """given: [(participant index, dh element)]; the first `threshold` are taken -> the dh element [x]R, or None"""
    taken = list(given)[:threshold]
    if len(taken) < threshold:
        return None
    indexes = [i for i, _ in taken]
    assert all(i < shares_n for i in indexes)
    denominators, scale = lagrange_coefficients(oracle, indexes)
    restored = oracle.point_multi_mul(b"".join(denominators), b"".join(dh for _, dh in taken))
    return oracle.point_multi_mul(scale, restored)


def scaled_coefficients(oracle, indexes):
    """scale / denominator_i: the scalars the batch pass multiplies the shares with ([scale] sum [1/d_i] S_i = sum [scale / d_i] S_i)"""
    inverted, scale = lagrange_coefficients(oracle, indexes)
    return [oracle.sc_mul(scale, d) for d in inverted]


# ------------------------------------------------------------------ key sets and shares
class KeySet:
    """A Shamir key set as test_threshold_tally_end_to_end makes it: secret = the polynomial at 0, participant i holds f(i + 1)"""

    def __init__(self, oracle, shares_n, threshold, seed):
        rnd = random.Random(seed)
        self.shares, self.threshold = shares_n, threshold
        coeffs = [rnd.randrange(L) for _ in range(threshold)]
        f = lambda x: sum(c * pow(x, k, L) for k, c in enumerate(coeffs)) % L
        self.secret = coeffs[0]
        self.sks = [f(i + 1) for i in range(shares_n)]
        self.shared_key = oracle.point_mul_generator(sc(self.secret))
        self.part_keys = [oracle.point_mul_generator(sc(s)) for s in self.sks]

    def dh(self, oracle, i, R):
        """participant i's share of the ciphertext with random element R (the element alone, without its proof)"""
        return oracle.point_multi_mul(sc(self.sks[i]), R)

    def item(self, oracle, i, R, rng):
        """the 128-byte item: R || dh || challenge || response, proven by the oracle"""
        return R + oracle.decryption_share_new(sc(self.sks[i]), R, self.shares, self.threshold, self.shared_key, i, rng)

    def plain_item(self, oracle, i, R):
        """an item without a proof (zero challenge and response): what the combine pass reads of an item is R and dh only"""
        return R + self.dh(oracle, i, R) + bytes(64)


def ciphertexts(oracle, key_set, counts, seed):
    """ElGamal ciphertexts of the given counts under the shared key: (R || B per count, [r])"""
    rnd = random.Random(seed)
    out = []
    for v in counts:
        r = rnd.randrange(1, L)
        R = oracle.point_mul_generator(sc(r))
        B = oracle.point_add(oracle.point_multi_mul(sc(r), key_set.shared_key), oracle.point_mul_generator(sc(v)))
        out.append(R + B)
    return out


# ------------------------------------------------------------------ the batch entry's rule, restated
def expected(oracle, shares_n, threshold, cts, indexes, columns, status=None, want_plain=True):
    """cts: [64 bytes]; columns[j][c]: the 128-byte item of column j for ciphertext c; status[j][c] or None.
    -> (dh, plain, combined, used, bad): per-ciphertext lists and the three counters"""
    dh, plain, combined, used, bad = [], [], [], [], [0, 0, 0]
    for c, ct in enumerate(cts):
        chosen = []
        for j, index in enumerate(indexes):
            if len(chosen) == threshold:
                break
            if status is not None and status[j][c] != OK:
                continue
            item = columns[j][c]
            if item[:32] != ct[:32]:
                bad[0] += 1
                continue
            chosen.append((index, item[32:64]))
        result = (ZERO32, ZERO32, 0, 0)
        if len(chosen) == threshold:
            undecodable = sum(1 for _, e in chosen if oracle.point_roundtrip(e) is None)
            bad[1] += undecodable
            if not undecodable:
                d = combine_shares(oracle, shares_n, threshold, chosen)
                mask = sum(1 << i for i, _ in chosen)
                if not want_plain:
                    result = (d, ZERO32, 1, mask)
                elif oracle.point_roundtrip(ct[32:]) is None:
                    bad[2] += 1
                else:
                    result = (d, oracle.point_add(ct[32:], d, True), 1, mask)
        for lst, v in zip((dh, plain, combined, used), result):
            lst.append(v)
    return dh, plain, combined, used, tuple(bad)
