"""Corpus of VALID ballots and proofs built from edge-case randomness (test infrastructure; built at test time by the oracle prover).

The verifiers' edge handling is reached only by inputs that are accepted: on the reject path a wrong intermediate point gives the
same verdict as a right one.  A prover chooses its own randomness, so honest ballots can be steered into the corners (the oracle's
scripted randomness, oracle.Script, pins a draw by its role):

- a ring nonce of 0 makes the recomputed commitments (R_G, R_K) of the actual index the identity;
- encryption randomness r = 0 makes the random element the identity (and the ciphertext (O, O) for a 0); 1 and l - 1 make it +-G;
- with r = 0 the actual index's response equals the nonce, so every response of that ring can be set to a chosen scalar: 0, 1,
  l - 1 and the scalars whose comb digits sit on the corners of the fixed-base tables (20- and 24-bit windows), both as c and as
  2c mod l because the equations are evaluated with halved scalars;
- r summing to 0 over the options makes the sum proof of a single-choice ballot run over the identity;
- two ballots with r and l - r on the same choices cancel in the tally;
- a decryption share of a tally slot whose random element is the identity has the identity as its log base.

Keys: the golden key (ChaChaRng 12345, the reference's snapshots) and G, -G, [2]G (secret keys 1, l - 1, 2).

What cannot be steered: every challenge is a hash output.  The per-ballot comb digits (challenge x ciphertext base) and the digits
of the challenge-dependent terms are therefore uniformly random here, never corners.  A response at the ACTUAL index equals
c * r + nonce, so it is chosen only when r = 0.

Not every bit of an accepted edge ballot is bound to its verdict.  In a ring whose ciphertext has r = 0 and whose actual index is
the last one, the last commitments ([s]G - [e]R, [s]K - [e](B - x)) do not depend on the challenge e, so the free responses before
them are unbound: flipping one leaves the ballot valid, in the reference as in the oracle.  The common challenge is always bound
(the verifier compares it with the recomputed one), so tamper tests that must reject flip it (Family.challenge_item).

Every Edge names what it reaches: `needs` = minimum oracle.diag() counts while the oracle verifies it alone, `items` = 32-byte items
of the packed ballot that must hold given bytes (the steered responses and ciphertext elements).
"""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field

from oracle import oracle as o

L = o.L
IDENTITY = bytes(32)
KEY_NAMES = ("golden", "G", "-G", "2G")
_SECRET = {"G": 1, "-G": L - 1, "2G": 2}


def sc(x: int) -> bytes:
    return (x % L).to_bytes(32, "little")


def key(name: str) -> bytes:
    if name == "golden":
        return o.keypair_from_seed(12345)[1]
    return o.point_mul_generator(sc(_SECRET[name]))


def element(k: int) -> bytes:
    return o.point_mul_generator(sc(k))


# the digit list of test_comb_tables_selfcheck_and_digit_corners, for 20-bit windows and its analogue for 24-bit ones
def _digits(bits: int):
    return [1, 2, 63, 64, 65, 127, 128, 129, 2 ** (bits - 1) - 1, 2 ** (bits - 1), 2 ** (bits - 1) + 1, 2**bits - 1, 2**bits - 64,
            2**bits - 65]


@functools.lru_cache(None)
def corner_scalars() -> tuple:
    """0, 1, l - 1 and every digit corner in every window of the 20- and 24-bit combs, each as c and as 2c mod l."""
    cs = [0, 1, L - 1]
    for bits in (20, 24):
        windows = (254 + bits - 1) // bits
        cs += [(d << (bits * w)) % L for w in range(windows) for d in _digits(bits)]
        cs.append(sum((2**bits - 1) << (bits * w) for w in range(windows)) % L)
    out = []
    for c in cs:
        for v in (c, 2 * c % L):
            if v not in out:
                out.append(v)
    return tuple(out)


@dataclass
class Edge:
    name: str
    ballot: bytes
    needs: dict = field(default_factory=dict)
    items: dict = field(default_factory=dict)


@dataclass
class Family:
    """One election (or proof kind) under one key, with its edge ballots.  kind: single, multi, qv, zero, bool, range, share."""
    name: str
    kind: str
    key_name: str
    key: bytes
    n_options: int = 0
    credits: int = 0
    edges: list = field(default_factory=list)
    extra: dict = field(default_factory=dict)
    oracle_params: object = None

    @property
    def size(self) -> int:
        return len(self.edges[0].ballot)

    @property
    def challenge_item(self) -> int:
        """Item index of a challenge that the verdict always depends on (the first ring proof's common challenge, or the
        log-equality challenge)."""
        if self.kind in ("single", "multi"):
            return 2 * self.n_options
        if self.kind == "qv":
            return 2 * len(self.oracle_params.vote_range.rings)
        if self.kind == "range":
            return 2 * len(self.extra["range"].rings)
        return 2

    @property
    def tallies(self) -> bool:
        return self.kind in ("single", "multi", "qv")

    def verify(self, ballot: bytes) -> int:
        p = self.oracle_params
        if self.kind in ("single", "multi", "qv"):
            return p.verify(ballot)
        if self.kind == "zero":
            return p.verify_zero(ballot)
        if self.kind == "bool":
            return p.verify_bool(ballot)
        if self.kind == "range":
            return p.verify_range(self.extra["range"], ballot)
        x = self.extra
        return o.decryption_share_verify(x["participant_key"], x["shares"], x["threshold"], self.key, x["index"], ballot)

    def tally(self, ballots: bytes, statuses) -> bytes:
        return self.oracle_params.tally(ballots, statuses)

    def gpu_params(self, eg, ctx):
        """The HIP verifier of this family; verify_batch(ballots) -> status words (and the tally for elections)."""
        if self.kind in ("single", "multi"):
            return eg.ChoiceParams(ctx, self.key, self.n_options, self.kind == "single")
        if self.kind == "qv":
            return eg.QuadraticVotingParams(ctx, self.key, self.n_options, self.credits)
        if self.kind == "zero":
            return eg.PublicKeyVerifier(ctx, self.key, eg.PublicKeyVerifier.ZERO)
        if self.kind == "bool":
            return eg.PublicKeyVerifier(ctx, self.key, eg.PublicKeyVerifier.BOOL)
        if self.kind == "range":
            return eg.PublicKeyVerifier(ctx, self.key, eg.PublicKeyVerifier.RANGE, self.credits)
        x = self.extra
        return eg.DecryptionShareVerifier(ctx, self.key, x["shares"], x["threshold"], x["index"], x["participant_key"])

    def random_ballots(self, seed: int, n: int) -> bytes:
        """n ordinary ballots of this election (uniform ChaCha randomness), for mixing with the edge ones."""
        p = self.oracle_params
        if self.kind == "qv":
            return p.generate_batch(seed, 0, n, threads=8)
        return p.generate_batch(seed, 0, n, n_selected=3 if self.kind == "multi" else 0, threads=8)


def scripted(pins, make):
    """make() under a script; every pinned role must have been drawn (the pins hit whatever the draw order)."""
    with o.Script(pins) as s:
        out = make()
    drawn = {(name, scope, i, k) for name, scope, i, k in s.trace}
    missed = [p for p in pins if tuple(list(p) + [0] * (4 - len(p))) not in drawn]
    assert not missed, f"pinned roles never drawn: {missed}"
    return out


def _chunks(xs, n):
    return [xs[i : i + n] for i in range(0, len(xs), n)]


# ------------------------------------------------------------------ choice elections
def _choice_family(name, key_name, n, single, corner_stride):
    pk = key(key_name)
    fam = Family(name, "single" if single else "multi", key_name, pk, n_options=n)
    op = fam.oracle_params = o.ChoiceParams(pk, n, single)
    rnd = random.Random(f"{name}/{key_name}")
    ring0 = 2 * n                                   # item index of the common challenge; responses follow, 2 per ring
    resp = lambda j, k: ring0 + 1 + 2 * j + k       # noqa: E731
    seeds = iter(range(1000, 10**6))

    def flags_with(j, actual):
        if single:
            f = [0] * n
            f[j if actual else (j + 1) % n] = 1
            return f
        others = [x for x in range(n) if x != j]
        chosen = set(rnd.sample(others, 3 - actual)) | ({j} if actual else set())
        return [int(x in chosen) for x in range(n)]

    def add(ename, flags, pins, needs=None, items=None):
        seed = next(seeds)
        b = scripted(pins, lambda: op.new_ballot(flags, o.rng_from_u64(seed)))
        fam.edges.append(Edge(ename, b, dict(needs or {}), dict(items or {})))

    rings = sorted({0, n // 2, n - 1})
    for j in rings:
        for actual in (0, 1):
            add(f"nonce0_ring{j}_actual{actual}", flags_with(j, actual), {("ring_nonce", 0, j): 0}, {"commitment": 2})
        for r in (0, 1, L - 1):
            add(f"r{'0' if r == 0 else '1' if r == 1 else 'l-1'}_opt{j}", flags_with(j, 0), {("ct_r", 0, j): r},
                {"ciphertext": 2} if r == 0 else {}, {2 * j: element(r)})
        for v in (0, 1, L - 1):                     # a free response (the index that is not the actual one) with r random
            add(f"free_response{'0' if v == 0 else '1' if v == 1 else 'l-1'}_ring{j}", flags_with(j, 1),
                {("ring_response", 0, j, 0): v}, {}, {resp(j, 0): sc(v)})
    if single:                                      # r summing to 0 over the options: the sum proof runs over the identity
        rs = [rnd.randrange(L) for _ in range(n - 1)]
        rs.append(-sum(rs) % L)
        add("r_sum0", flags_with(n - 1, 1), {("ct_r", 0, j): r for j, r in enumerate(rs)}, {"base": 2})
    # r = 0 everywhere: every response is chosen -> the comb-digit corners (and 0 / 1 / l - 1) as responses
    per = 2 * n + (1 if single else 0)
    corners = list(corner_scalars()[::corner_stride])
    for c, vals in enumerate(_chunks(corners, per)):
        vals = vals + [rnd.randrange(L) for _ in range(per - len(vals))]
        flags = flags_with(c % n, 1)
        pins = {("ct_r", 0, j): 0 for j in range(n)}
        items = {}
        for j in range(n):
            a = flags[j]                            # actual index of ring j: its response = nonce (r = 0)
            pins[("ring_nonce", 0, j)] = vals[2 * j]
            pins[("ring_response", 0, j, 1 - a)] = vals[2 * j + 1]
            items[resp(j, a)] = sc(vals[2 * j])
            items[resp(j, 1 - a)] = sc(vals[2 * j + 1])
        if single:
            pins[("logeq_nonce", 0)] = vals[-1]     # sum of r = 0: the sum proof's response = its nonce
            items[ring0 + 1 + 2 * n + 1] = sc(vals[-1])
        add(f"r0_corner_responses{c}", flags, pins, {"ciphertext": n, **({"base": 2} if single else {})}, items)
    # r = 0 and nonce 0 in one ring: identity ciphertext AND identity commitments, response 0
    add("r0_nonce0_ring0", flags_with(0, 0), {("ct_r", 0, 0): 0, ("ring_nonce", 0, 0): 0}, {"ciphertext": 2, "commitment": 2},
        {0: IDENTITY, 1: IDENTITY, resp(0, 0): sc(0)})
    # two ballots whose ciphertexts cancel slot by slot (r and l - r on the same choices)
    flags = flags_with(0, 1)
    rs = [rnd.randrange(1, L) for _ in range(n)]
    add("cancel_a", flags, {("ct_r", 0, j): r for j, r in enumerate(rs)})
    add("cancel_b", flags, {("ct_r", 0, j): L - r for j, r in enumerate(rs)})
    return fam


# ------------------------------------------------------------------ quadratic voting
def _qv_family(key_name, n, credits, corner_stride):
    pk = key(key_name)
    fam = Family(f"qv{n}x{credits}", "qv", key_name, pk, n_options=n, credits=credits)
    op = fam.oracle_params = o.QvParams(pk, n, credits)
    rnd = random.Random(f"qv/{key_name}")
    seeds = iter(range(2000, 10**6))
    vote_rings = len(op.vote_range.rings)
    full = [4, 2] + [0] * (n - 2)                   # sum of squares == credits (20)
    assert sum(v * v for v in full) == credits
    zeros = [0] * n

    def add(ename, votes, pins, needs=None, items=None):
        seed = next(seeds)
        b = scripted(pins, lambda: op.new_ballot(votes, o.rng_from_u64(seed)))
        fam.edges.append(Edge(ename, b, dict(needs or {}), dict(items or {})))

    vitem = lambda i: i * op.vote_size // 32        # noqa: E731  first item of vote i
    for votes, tag in ((zeros, "zero_votes"), (full, "full_credits")):
        add(f"{tag}_plain", votes, {})
        for i in sorted({0, n // 2, n - 1}):
            add(f"{tag}_value_r0_vote{i}", votes, {("value_r", i): 0}, {"ciphertext": 1}, {vitem(i): IDENTITY})
            add(f"{tag}_nonce0_vote{i}", votes, {("ring_nonce", i, vote_rings - 1): 0}, {"commitment": 2})
        add(f"{tag}_credit_r0", votes, {("value_r", n): 0}, {"base": 1}, {n * op.vote_size // 32: IDENTITY})
        add(f"{tag}_sumsq_nonces0", votes, {**{("sumsq_er", 0, i): 0 for i in range(n)}, **{("sumsq_ex", 0, i): 0 for i in range(n)},
                                            ("sumsq_ez",): 0}, {"commitment": 2 * n + 1})
        # no randomness at all: every ciphertext, partial and commitment of the ballot that can be the identity is
        pins = {("value_r", s): 0 for s in range(n + 1)}
        for s in range(n + 1):
            rings = vote_rings if s < n else len(op.credit_range.rings)
            for ring in range(rings):
                pins[("ct_r", s, ring)] = 0
                pins[("ring_nonce", s, ring)] = 0
        pins.update({("sumsq_er", 0, i): 0 for i in range(n)})
        pins.update({("sumsq_ex", 0, i): 0 for i in range(n)})
        pins[("sumsq_ez",)] = 0
        pins = {k: v for k, v in pins.items() if k[0] != "ct_r" or k[2] < (vote_rings if k[1] < n else len(op.credit_range.rings)) - 1}
        add(f"{tag}_all_randomness0", votes, pins, {"commitment": 2 * n + 2, "ciphertext": 2, "base": 1})
    # free responses of the vote rings at the corners (r random; the ring's actual index is not pinned)
    sizes = [s for s, _ in op.vote_range.rings]
    corners = list(corner_scalars()[::corner_stride])
    for c, vals in enumerate(_chunks(corners, n)):
        votes = [0] * n                             # vote 0: every ring's actual index is 0, responses 1.. are free
        pins, items = {}, {}
        for i, v in enumerate(vals):
            pins[("ring_response", i, 0, sizes[0] - 1)] = v
            items[vitem(i) + 2 * vote_rings + 1 + sizes[0] - 1] = sc(v)
        add(f"corner_free_responses{c}", votes, pins, {}, items)
    rs = [rnd.randrange(1, L) for _ in range(n)]
    add("cancel_a", full, {("value_r", i): r for i, r in enumerate(rs)})
    add("cancel_b", full, {("value_r", i): L - r for i, r in enumerate(rs)})
    return fam


# ------------------------------------------------------------------ PublicKey::encrypt_zero / _bool / _range, decryption shares
def _pk_families(key_name):
    pk = key(key_name)
    k = o.PublicKey(pk)
    fams = []
    seeds = iter(range(3000, 10**6))

    def add(fam, ename, make, pins, needs=None, items=None):
        seed = next(seeds)
        b = scripted(pins, lambda: make(o.rng_from_u64(seed)))
        fam.edges.append(Edge(ename, b, dict(needs or {}), dict(items or {})))

    z = Family("zero", "zero", key_name, pk, oracle_params=k)
    add(z, "plain", k.encrypt_zero, {})
    add(z, "r0", k.encrypt_zero, {("ct_r", 0, 0): 0}, {"base": 2}, {0: IDENTITY, 1: IDENTITY})
    add(z, "r1", k.encrypt_zero, {("ct_r", 0, 0): 1}, {}, {0: element(1), 1: pk})
    add(z, "nonce0", k.encrypt_zero, {("logeq_nonce",): 0}, {"commitment": 2})
    add(z, "r0_nonce0", k.encrypt_zero, {("ct_r", 0, 0): 0, ("logeq_nonce",): 0}, {"base": 2, "commitment": 2}, {3: sc(0)})
    fams.append(z)

    bo = Family("bool", "bool", key_name, pk, oracle_params=k)
    for v in (0, 1):
        mk = functools.partial(k.encrypt_bool, bool(v))
        add(bo, f"plain{v}", mk, {})
        add(bo, f"r0_value{v}", mk, {("ct_r", 0, 0): 0}, {"ciphertext": 2 - v})
        add(bo, f"rl-1_value{v}", mk, {("ct_r", 0, 0): L - 1}, {}, {0: element(L - 1)})
        add(bo, f"nonce0_value{v}", mk, {("ring_nonce", 0, 0): 0}, {"commitment": 2})
        add(bo, f"free_response_l-1_value{v}", mk, {("ring_response", 0, 0, 1 - v): L - 1}, {}, {4 - v: sc(L - 1)})
        add(bo, f"r0_responses01_value{v}", mk, {("ct_r", 0, 0): 0, ("ring_nonce", 0, 0): 1, ("ring_response", 0, 0, 1 - v): 0},
            {"ciphertext": 2 - v}, {3 + v: sc(1), 4 - v: sc(0)})
    fams.append(bo)

    bound = 100
    pr = o.PreparedRange(bound)
    ra = Family(f"range{bound}", "range", key_name, pk, credits=bound, oracle_params=k, extra={"range": pr})
    n_rings = len(pr.rings)
    for value in (0, 42, bound - 1):
        mk = functools.partial(k.encrypt_range, pr, value)
        add(ra, f"plain_v{value}", mk, {})
        add(ra, f"value_r0_v{value}", mk, {("value_r", 0): 0, **{("ct_r", 0, i): 0 for i in range(n_rings - 1)}},
            {"ciphertext": 2 * n_rings if value == 0 else n_rings}, {0: IDENTITY})
        add(ra, f"nonce0_v{value}", mk, {("ring_nonce", 0, i): 0 for i in range(n_rings)}, {"commitment": 2 * n_rings})
    fams.append(ra)

    # decryption shares: participant key [x]G of a 2-of-3 key set over this key; the ciphertext's random element is chosen
    sh = Family("share", "share", key_name, pk, oracle_params=None,
                extra={"shares": 3, "threshold": 2, "index": 1, "participant_key": element(777)})

    def share(r_elem):
        return lambda rng: r_elem + o.decryption_share_new(sc(777), r_elem, 3, 2, pk, 1, rng)

    for tag, r_elem in (("R_random", element(98765)), ("R_identity", IDENTITY), ("R_G", element(1)), ("R_-G", element(L - 1))):
        add(sh, f"{tag}_plain", share(r_elem), {}, {"base": 2} if r_elem == IDENTITY else {})
        add(sh, f"{tag}_nonce0", share(r_elem), {("logeq_nonce",): 0}, {"commitment": 2})
    fams.append(sh)
    return fams


# ------------------------------------------------------------------ the corpus
FAMILY_NAMES = ("single2", "single5", "single16", "multi3of16", "multi20", "qv5x20", "zero", "bool", "range100", "share")


@functools.lru_cache(None)
def family(name: str, key_name: str = "golden") -> Family:
    stride = 1 if key_name == "golden" and name in ("single2", "single5") else 7
    if name.startswith("single"):
        return _choice_family(name, key_name, int(name[6:]), True, stride)
    if name == "multi3of16":
        return _choice_family(name, key_name, 16, False, stride)
    if name == "multi20":                           # 40 deferred commitments per stage: k_encode_batch runs two groups
        return _choice_family(name, key_name, 20, False, 3 * stride)
    if name == "qv5x20":
        return _qv_family(key_name, 5, 20, 2 if key_name == "golden" else 9)
    return {f.name: f for f in _pk_families(key_name)}[name]


def tamper(ballot: bytes, seed: int, item: int | None = None) -> bytes:
    """One bit flipped in one 32-byte item, a random one unless given (never in the top byte, so that most flips keep a scalar
    canonical)."""
    rnd = random.Random(seed)
    b = bytearray(ballot)
    item = rnd.randrange(len(b) // 32) if item is None else item
    b[32 * item + rnd.randrange(31)] ^= 1 << rnd.randrange(8)
    return bytes(b)
