"""Pure-Python model of the receipt log (eg_merkle_*), written from the text of RFC 6962 2.1 / 2.1.1 and RFC 9162 2.1.3.2 with hashlib
only.  Every expected value of tests/test_merkle_cpu.py and tests/test_gpu_merkle.py comes from here.

H(x) = the first 32 bytes of SHA-512(x).  leaf = H(0x00 || prefix || msg || extra), node(l, r) = H(0x01 || l || r), MTH({}) = H("").
MTH and PATH are the RFC's recursions (split at k, the largest power of two below n): independent of the kernels' bottom-up form, which
`levels` restates so that the two can be compared."""
import hashlib

BAD_INDEX, BAD_LENGTH, MISMATCH = 1, 2, 3
LEAF_NONE = (1 << 64) - 1
NO_PATH = 0xFFFFFFFF
LEAVES_MAX = 1 << 31


def H(x: bytes) -> bytes:
    return hashlib.sha512(x).digest()[:32]


def leaf_hash(msg: bytes, prefix: bytes = b"", extra: bytes = b"") -> bytes:
    return H(b"\x00" + prefix + msg + extra)


def node_hash(left: bytes, right: bytes) -> bytes:
    return H(b"\x01" + left + right)


def _split(n: int) -> int:
    """the largest power of two smaller than n (n > 1)"""
    k = 1
    while 2 * k < n:
        k *= 2
    return k


def mth(leaves) -> bytes:
    """RFC 6962 2.1 over a list of leaf HASHES (the log's entries are hashed already)"""
    n = len(leaves)
    if n == 0:
        return H(b"")
    if n == 1:
        return leaves[0]
    k = _split(n)
    return node_hash(mth(leaves[:k]), mth(leaves[k:]))


def path(m: int, leaves) -> list:
    """RFC 6962 2.1.1: PATH(m, D[n]), bottom-up"""
    n = len(leaves)
    assert 0 <= m < n
    if n == 1:
        return []
    k = _split(n)
    if m < k:
        return path(m, leaves[:k]) + [mth(leaves[k:])]
    return path(m - k, leaves[k:]) + [mth(leaves[:k])]


def depth(n: int) -> int:
    return (n - 1).bit_length() if n > 1 else 0


def path_len(i: int, n: int) -> int:
    """closed form: one entry per level at which the sibling i ^ 1 exists"""
    length = 0
    while n > 1:
        if (i ^ 1) < n:
            length += 1
        i >>= 1
        n = (n + 1) >> 1
    return length


def levels(leaves) -> list:
    """the bottom-up form: [level 0, level 1, ...] up to the single root (an empty or one-leaf log has level 0 only)"""
    out = [list(leaves)]
    while len(out[-1]) > 1:
        a = out[-1]
        out.append([node_hash(a[2 * i], a[2 * i + 1]) if 2 * i + 1 < len(a) else a[2 * i] for i in range((len(a) + 1) // 2)])
    return out


def level_count(n: int, level: int) -> int:
    return -(-n // (1 << level))


def node_store(leaves) -> bytes:
    """levels 1 .. depth back to back"""
    return b"".join(b"".join(lv) for lv in levels(leaves)[1:])


def rfc9162_check(i: int, n: int, leaf: bytes, proof, root: bytes) -> int:
    """RFC 9162 2.1.3.2, with the verdicts of the library: the first failure in the order index, length, root"""
    if i >= n:
        return BAD_INDEX
    fn, sn, r = i, n - 1, leaf
    for p in proof:
        if sn == 0:
            return BAD_LENGTH                 # a path that is too long
        if fn & 1 or fn == sn:
            r = node_hash(p, r)
            if not fn & 1:
                while not fn & 1 and fn != 0:
                    fn >>= 1
                    sn >>= 1
        else:
            r = node_hash(r, p)
        fn >>= 1
        sn >>= 1
    if sn != 0:
        return BAD_LENGTH                     # a path that is too short
    return 0 if r == root else MISMATCH


def check(i: int, n: int, leaf: bytes, proof, root: bytes) -> int:
    """the verdict rule: the length is judged BEFORE any path byte is looked at"""
    if i >= n:
        return BAD_INDEX
    if len(proof) != path_len(i, n):
        return BAD_LENGTH
    return rfc9162_check(i, n, leaf, proof, root)


def leaves_pass(msgs, prefix=b"", extras=None, status=None, n_prior=0, log_cap=None):
    """the leaf pass over a batch: dict(leaf_index, leaves_out, appended, log_count, found)"""
    n = len(msgs)
    part = [status is None or status[b] == 0 for b in range(n)]
    hashes = [leaf_hash(msgs[b], prefix, extras[b] if extras else b"") if part[b] else bytes(32) for b in range(n)]
    index, rank = [], 0
    for b in range(n):
        index.append(n_prior + rank if part[b] else LEAF_NONE)
        rank += part[b]
    appended = [hashes[b] for b in range(n) if part[b]]
    fits = log_cap is None or n_prior + rank <= log_cap
    return {"leaf_index": index, "leaves_out": hashes, "appended": appended if fits else [], "log_count": n_prior + (rank if fits else 0),
            "found": [rank, 0 if fits else 1]}
