"""Pure-Python model of the receipt log's audit entries (eg_merkle_heads / _consistency / _consistency_check), written from the text of
RFC 9162 2.1.4.1 (PROOF / SUBPROOF, the recursion) and 2.1.4.2 (the literal verification algorithm) with hashlib only, on top of
tests/merkle_ref.py.  Every expected value of tests/test_merkle_audit_cpu.py and tests/test_gpu_merkle_audit.py comes from here.

The forms the kernels use (the fold over the bits of m for a past head, the proof read out of the bottom-up levels, the check as a walk
over the levels) are restated beside the RFC's, so that the two can be compared; `self_check` does that."""
import merkle_ref as M

BAD_INDEX, BAD_LENGTH, MISMATCH, MISMATCH_OLD = M.BAD_INDEX, M.BAD_LENGTH, M.MISMATCH, 4
NO_PATH = M.NO_PATH


# ------------------------------------------------------------------ the RFC's forms
def subproof(m: int, leaves, b: bool) -> list:
    """RFC 9162 2.1.4.1: SUBPROOF(m, D_n, b) over leaf HASHES"""
    n = len(leaves)
    assert 0 < m <= n
    if m == n:
        return [] if b else [M.mth(leaves)]
    k = M._split(n)
    if m <= k:
        return subproof(m, leaves[:k], b) + [M.mth(leaves[k:])]
    return subproof(m - k, leaves[k:], False) + [M.mth(leaves[:k])]


def proof(m: int, leaves) -> list:
    """PROOF(m, D_n) = SUBPROOF(m, D_n, true)"""
    return subproof(m, leaves, True)


def rfc9162_consistency(first: int, second: int, first_hash: bytes, second_hash: bytes, path) -> int:
    """RFC 9162 2.1.4.2, step by step, for 0 < first < second, with the verdicts of the library: a path that is too short or too long is
    BAD_LENGTH; then the old root is judged before the new one"""
    assert 0 < first < second
    path = list(path)
    if not path:                                                          # 1
        return BAD_LENGTH
    if first & (first - 1) == 0:                                          # 2: an exact power of two
        path = [first_hash] + path
    fn, sn = first - 1, second - 1                                        # 3
    while fn & 1:                                                         # 4
        fn >>= 1
        sn >>= 1
    fr = sr = path[0]                                                     # 5
    for c in path[1:]:                                                    # 6
        if sn == 0:
            return BAD_LENGTH
        if fn & 1 or fn == sn:
            fr = M.node_hash(c, fr)
            sr = M.node_hash(c, sr)
            if not fn & 1:
                while not fn & 1 and fn != 0:
                    fn >>= 1
                    sn >>= 1
        else:
            sr = M.node_hash(sr, c)
        fn >>= 1
        sn >>= 1
    if sn != 0:                                                           # 7
        return BAD_LENGTH
    if fr != first_hash:
        return MISMATCH_OLD
    return 0 if sr == second_hash else MISMATCH


# ------------------------------------------------------------------ the library's rule
def _seed(m: int):
    """(level, node) of the last complete piece of the old tree: m = (node + 1) 2^level"""
    node, level = m - 1, 0
    while node & 1:
        node >>= 1
        level += 1
    return level, node


def consistency_len(m: int, n: int) -> int:
    """the closed form: NO_PATH for m == 0 or m > n, 0 for m == n, else the seed (if any) and one entry per level at which the sibling exists"""
    if m == 0 or m > n:
        return NO_PATH
    if m == n:
        return 0
    level, node = _seed(m)
    length = 1 if node else 0
    count = M.level_count(n, level)
    while count > 1:
        if (node ^ 1) < count:
            length += 1
        node >>= 1
        count = (count + 1) >> 1
    return length


def check(m: int, n: int, old_root: bytes, path, root: bytes) -> int:
    """the verdict rule: index, then the length BEFORE any proof byte is looked at, then the old root, then the new root"""
    if m == 0 or m > n:
        return BAD_INDEX
    if len(path) != consistency_len(m, n):
        return BAD_LENGTH
    if m == n:
        return 0 if old_root == root else MISMATCH
    return rfc9162_consistency(m, n, old_root, root, path)


# ------------------------------------------------------------------ the forms of the kernels, over the bottom-up levels of merkle_ref
def past_head(m: int, levels) -> bytes:
    """the head of the first m leaves out of the levels of a larger tree: the complete subtrees that the bits of m name, folded on the left"""
    if m == 0:
        return M.H(b"")
    acc, x, level = None, m, 0
    while x:
        if x & 1:
            piece = levels[level][x - 1]
            acc = piece if acc is None else M.node_hash(piece, acc)
        x >>= 1
        level += 1
    return acc


def store_proof(m: int, levels) -> list:
    """the proof of (m, N) read out of the levels: the seed, then the audit path of the seed's node"""
    n = len(levels[0])
    assert 0 < m <= n
    if m == n:
        return []
    level, node = _seed(m)
    out = [levels[level][node]] if node else []
    while len(levels[level]) > 1:
        if (node ^ 1) < len(levels[level]):
            out.append(levels[level][node ^ 1])
        node >>= 1
        level += 1
    return out


def walk_check(m: int, n: int, old_root: bytes, path, root: bytes) -> int:
    """the check as the lane does it: driven by (m, N) alone once the length is exact"""
    if m == 0 or m > n:
        return BAD_INDEX
    if len(path) != consistency_len(m, n):
        return BAD_LENGTH
    fr = sr = old_root
    if m < n:
        level, node = _seed(m)
        k = 0
        if node:
            fr = sr = path[0]
            k = 1
        count = M.level_count(n, level)
        while count > 1:
            if (node ^ 1) < count:
                c = path[k]
                k += 1
                if node & 1:
                    fr, sr = M.node_hash(c, fr), M.node_hash(c, sr)
                else:
                    sr = M.node_hash(sr, c)
            node >>= 1
            count = (count + 1) >> 1
    if fr != old_root:
        return MISMATCH_OLD
    return 0 if sr == root else MISMATCH


def flip(x: bytes, bit: int) -> bytes:
    return x[:bit // 8] + bytes([x[bit // 8] ^ (1 << (bit % 8))]) + x[bit // 8 + 1:]


def self_check(leaves, n_max: int) -> int:
    """every 1 <= m <= N <= n_max: the proof proves, the recursion equals the store form, the length equals the closed form, the past head
    equals MTH of the prefix, truncated and lengthened proofs fail, a flipped bit in any entry or either root fails with the right one of
    the two mismatch verdicts, and the walk agrees with the literal algorithm throughout.  Returns the number of proofs looked at"""
    seen = 0
    heads = [M.mth(leaves[:m]) for m in range(n_max + 1)]
    for n in range(1, n_max + 1):
        lv = M.levels(leaves[:n])
        root = heads[n]
        assert past_head(0, lv) == M.H(b"") == heads[0]
        for m in range(1, n + 1):
            p = proof(m, leaves[:n])
            assert p == store_proof(m, lv), (m, n)
            assert len(p) == consistency_len(m, n) <= M.depth(n) + 1, (m, n)
            assert past_head(m, lv) == heads[m], (m, n)
            assert check(m, n, heads[m], p, root) == 0 == walk_check(m, n, heads[m], p, root), (m, n)
            seen += 1
            if m == n:
                assert p == [] and check(m, n, heads[m], [bytes(32)], root) == BAD_LENGTH
                assert check(m, n, flip(root, m % 256), [], root) == MISMATCH == walk_check(m, n, flip(root, m % 256), [], root)
                continue
            # lengths: the literal algorithm alone refuses them too
            for bad in (p[:-1], p[1:], p + [bytes(32)], p + [p[-1]]):
                assert check(m, n, heads[m], bad, root) == BAD_LENGTH == walk_check(m, n, heads[m], bad, root), (m, n)
            assert rfc9162_consistency(m, n, heads[m], root, p[:-1]) != 0 and rfc9162_consistency(m, n, heads[m], root, p + [bytes(32)]) == BAD_LENGTH
            # one flipped bit in every entry and in either root: which root is reported
            level, node = _seed(m)
            for k in range(len(p)):
                bent = p[:k] + [flip(p[k], (m + 7 * k) % 256)] + p[k + 1:]
                got = check(m, n, heads[m], bent, root)
                assert got == walk_check(m, n, heads[m], bent, root) and got in (MISMATCH_OLD, MISMATCH), (m, n, k)
                if k == 0 and node:
                    assert got == MISMATCH_OLD, (m, n)                      # the seed feeds both chains
            old_bent = check(m, n, flip(heads[m], n % 256), p, root)
            assert old_bent == walk_check(m, n, flip(heads[m], n % 256), p, root)
            assert old_bent == (MISMATCH_OLD if node else MISMATCH), (m, n)   # without a seed the old root IS the start of both chains
            assert check(m, n, heads[m], p, flip(root, m % 256)) == MISMATCH == walk_check(m, n, heads[m], p, flip(root, m % 256)), (m, n)
        for m in (0, n + 1, 1 << 40):
            assert check(m, n, heads[0], [], root) == BAD_INDEX == walk_check(m, n, heads[0], [], root) and consistency_len(m, n) == NO_PATH
    return seen
