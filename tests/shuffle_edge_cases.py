"""Cases of the shuffle verifier's chain kernel beyond what an honest prover makes (tests/test_shuffle_edges_cpu.py and
tests/test_gpu_shuffle_edges.py share them; tests/shuffle_cases.py has the honest shuffle and its twins).

PASSING ROWS AT THE EDGES.  The verifier takes the commitment key as an argument, so a test may hand in H_0 = [h]G with h known (a
trapdoor).  With c^_i = [a_i]G and t^_i = [tau_i]G chosen freely the challenge x is fixed by the transcript, and CHAIN of row i,
    t^_i = [-x]c^_i + [s^_i]G + [s'_i]c^_(i-1),        is        tau_i = -x a_i + s^_i + s'_i a_prev        (a_prev = a_(i-1), or h for row 0)
in known scalars: fix s'_i = e and solve s^_i, or fix s^_i = e and solve s'_i (a_prev != 0).  build() makes a twin of that kind from a
list of row specifications, in the form that shuffle_cases.judge and the runners of the test files take.  in, out, c and the head are
arbitrary elements: every T bit fails, no row does.  Both scalars zero under a general c^_i would need tau_i = -x a_i while x is a hash
over t^_i: not reachable, and not forced; with c^_i and t^_i the identity it is an ordinary row of the list (s' = 0 gives s^ = 0).

WHAT A TAMPERED PROOF MUST GIVE.  x hashes c, c^, t^ and the head, never s^ or s': a changed s^_k moves nothing but CHAIN of row k, a
changed s'_k CHAIN of row k and the T sums.  The expect_* functions state the whole answer (verdict, rows, found) of such twins;
tests/test_shuffle_edges_cpu.py holds them against the model with the oracle judging, so the GPU tests may rest on them where a whole
judgement by the oracle costs too much."""
import random

import shuffle_cases as SC
import shuffle_ref as m

L = m.L
NONE4 = [0, 0, m.NONE, m.NONE]
EIGHTS = int("8" * 63, 16)                  # 0x0888...8: every one of the 63 low radix-16 digits is 8, every recoded digit carries
SEVENS = int("7" * 63, 16)
EDGES = {
    "0": 0, "1": 1, "2": 2, "7": 7, "8": 8, "9": 9, "15": 15, "16": 16,
    "2^128-1": (1 << 128) - 1, "2^128": 1 << 128,
    "2^252-1": (1 << 252) - 1,              # = 0x0f...f, 63 digits f
    "2^252": 1 << 252,
    "(l-1)/2": (L - 1) // 2, "(l+1)/2": (L + 1) // 2,
    "l-2^128": L - (1 << 128), "l-8": L - 8, "l-2": L - 2, "l-1": L - 1,
    "0x0888..8": EIGHTS, "0x0777..7": SEVENS,
}
ROLES = ("sprime", "shat")                  # which of the two scalars of the row is the edge; the other one is solved
C_KINDS = ("identity", "random", "prev", "neg_prev", "G", "neg_G", "8G")
T_KINDS = ("random", "identity", "G")
SPACER = {"c": "random", "t": "random", "role": "sprime", "edge": None}        # s' random: the row behind an identity c^
TILE_EDGE_ROWS = (61, 62, 63, 64, 125, 126)                                    # the lanes that end and begin a tile of 63 rows


def product_specs():
    """every (t^ kind, scalar edge, role, c^ kind), the c^ kind running fastest.  A row whose predecessor is the identity cannot have
    s' solved, so a spacer follows every identity c^: 8 rows per (t^, edge, role), 960 in all."""
    out = []
    for t in T_KINDS:
        for edge in EDGES:
            for role in ROLES:
                for c in C_KINDS:
                    out.append({"c": c, "t": t, "role": role, "edge": edge})
                    if c == "identity":
                        out.append(dict(SPACER))
    return out


def cover_specs():
    """the short list for the slow runners: every (edge, role) once, the c^ and t^ kinds cycling against them with periods 7 and 3, so
    every kind of either appears several times; spacers as above"""
    out = []
    k = 0
    for edge in EDGES:
        for role in ROLES:
            c = C_KINDS[k % 7]
            out.append({"c": c, "t": T_KINDS[k % 3], "role": role, "edge": edge})
            if c == "identity":
                out.append(dict(SPACER))
            k += 1
    return out


def window(specs, n, offset):
    """n rows of the list, repeated, from `offset` on"""
    return [specs[(offset + r) % len(specs)] for r in range(n)]


def _alpha(kind, prev, rnd):
    return rnd() if kind == "random" else {"identity": 0, "prev": prev, "neg_prev": -prev % L, "G": 1, "neg_G": L - 1, "8G": 8}[kind]


def build(be, specs, h, K, seed, prefix=SC.PREFIX, name="edges"):
    """The twin dict(name, ins, outs, K, key, prefix, proof) of the row specifications, with H_0 = [h]G, and beside it what the
    tests look at: specs (as built), alpha (the logarithms of c^), alpha_prev, shat, sprime, x.  A specification is
    dict(c = one of C_KINDS, t = one of T_KINDS, role = "sprime" | "shat", edge = a name of EDGES or None for a random scalar)."""
    n = len(specs)
    rng = random.Random(seed)
    rnd = lambda: rng.getrandbits(512) % (L - 1) + 1
    assert h % L
    alpha, alpha_prev, tau, prev = [], [], [], h % L
    for s in specs:
        a = _alpha(s["c"], prev, rnd)
        alpha.append(a)
        alpha_prev.append(prev)
        tau.append(rnd() if s["t"] == "random" else {"identity": 0, "G": 1}[s["t"]])
        prev = a
    pts = be.mul_generator([h] + [rnd() for _ in range(n)] + alpha + tau + [rnd() for _ in range(5 * n + 5)])
    key, chat, that = pts[:n + 1], pts[n + 1:2 * n + 1], pts[2 * n + 1:3 * n + 1]
    rest = pts[3 * n + 1:]
    ins = [rest[i] + rest[n + i] for i in range(n)]
    outs = [rest[2 * n + i] + rest[3 * n + i] for i in range(n)]
    c, head = rest[4 * n:5 * n], rest[5 * n:]
    seed1, _ = m.challenges_u(n, ins, outs, K, key, prefix, c)
    x = m.challenge_x(n, seed1, chat, that, head)
    shat, sprime = [], []
    for i, s in enumerate(specs):
        e = rnd() if s["edge"] is None else EDGES[s["edge"]]
        if s["role"] == "sprime":
            sprime.append(e)
            shat.append((tau[i] + x * alpha[i] - e * alpha_prev[i]) % L)
        else:
            if alpha_prev[i] == 0:
                raise ValueError(f"row {i}: s' cannot be solved behind the identity")
            shat.append(e)
            sprime.append((tau[i] + x * alpha[i] - e) * pow(alpha_prev[i], -1, L) % L)
    proof = b"".join(head) + b"".join(m.sc(rnd()) for _ in range(4)) + b"".join(c) + b"".join(chat) + b"".join(that) + \
        b"".join(m.sc(v) for v in shat) + b"".join(m.sc(v) for v in sprime)
    return {"name": name, "ins": ins, "outs": outs, "K": K, "key": key, "prefix": prefix, "proof": proof,
            "specs": list(specs), "alpha": alpha, "alpha_prev": alpha_prev, "shat": shat, "sprime": sprime, "x": x}


def twin_of(t):
    """the part of a built case that the judge and the runners read"""
    return {k: t[k] for k in ("name", "ins", "outs", "K", "key", "prefix", "proof")}


# ---------------------------------------------------------------------------------------------------------------- tampers and what they give
def scalar_of(proof, n, section, k):
    return int.from_bytes(SC.get(proof, n, section, k), "little")


def plus_one(proof, n, section, rows):
    """s^_k (section "shat") or s'_k ("sprime") replaced by itself + 1 mod l in every row of `rows`; nothing is proved again"""
    for k in rows:
        proof = SC.put(proof, n, section, k, m.sc(scalar_of(proof, n, section, k) + 1))
    return proof


def with_rows(t, name, section, rows, value=None):
    """the twin with section[k] + 1 mod l (value = None) or `value` (32 bytes) in the rows"""
    n = len(t["ins"])
    proof = t["proof"]
    if value is None:
        proof = plus_one(proof, n, section, rows)
    else:
        for k in rows:
            proof = SC.put(proof, n, section, k, value)
    return dict(twin_of(t), name=name, proof=proof)


def expect_chain_rows(n, rows):
    """rows and found when exactly `rows` fail CHAIN and no encoding is bad"""
    rows = sorted(set(rows))
    return [m.ROW_CHAIN if i in set(rows) else 0 for i in range(n)], [0, len(rows), m.NONE, rows[0] if rows else m.NONE]


def expect_shat_plus_one(n, rows, mask_before=0):
    """(verdict, rows, found) of a proof with the verdict mask_before (no CHAIN, no BAD_ENCODING) after s^_k += 1 in `rows`"""
    assert not mask_before & (m.CHAIN | m.BAD_ENCODING)
    words, found = expect_chain_rows(n, rows)
    return (mask_before | m.CHAIN) if found[1] else mask_before, words, found


def expect_scalar_is_l(n, k):
    """s^_k or s'_k := l in an accepted proof: the row is bad and is not evaluated; no other row reads it"""
    return m.BAD_ENCODING, [m.ROW_BAD if i == k else 0 for i in range(n)], [1, 0, k, m.NONE]


def expect_chat_not_a_point(n, k):
    """c^_k := 32 bytes that decode to nothing, in an accepted proof: row k is bad, row k + 1 has no predecessor to be evaluated against
    and stays 0, and every other row fails CHAIN, because c^ is hashed into x"""
    chain = [i for i in range(n) if i not in (k, k + 1)]
    rows = [m.ROW_BAD if i == k else m.ROW_CHAIN if i in set(chain) else 0 for i in range(n)]
    return m.BAD_ENCODING, rows, [1, len(chain), k, chain[0] if chain else m.NONE]


LL = L.to_bytes(32, "little")


def edge_rows(n):
    """row 0, the rows at the tiles' edges and the last row"""
    return sorted({k for k in (0, *TILE_EDGE_ROWS, n - 1) if k < n})
