"""The GPU provers of the zero, bool, range, sum-of-squares and decryption-share proofs (csrc/prover_kernels.cuh: k_zero_prove,
k_range_prove, k_sumsq_prove, k_share_prove) and, with the items they make, the five verifiers at a size the oracle's CPU provers
could never feed: the reference's snapshots byte for byte, byte parity with the oracle's provers over thousands of seeds, 100 000
generated items per kind with a tenth tampered against the oracle's verdicts, bad inputs, and the neighbours left alone.
Bit-exact: integer and byte work."""
import ctypes as C
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493
BAD_POINT_BYTES = b"\x01" + bytes(31)      # an odd ("negative") field element never is a ristretto255 encoding
BAD_ARG = -3                               # include/eg_hip.h: EG_ERR_BAD_ARG
ZERO, BOOL, RANGE, SHARE, SUMSQ = 0, 1, 2, 3, 4


def sc(x):
    return (x % L).to_bytes(32, "little")


@pytest.fixture(scope="module")
def eg():
    import elastic_elgamal_amd as m

    return m


@pytest.fixture(scope="module")
def ctx(eg):
    c = eg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pk(oracle, golden):
    return oracle.keypair_from_seed(golden["seed"])[1]


def pmap(fn, seq, workers=16):
    """fn over seq on threads: the oracle is a C library behind ctypes (the interpreter lock is released inside it) with thread-local
    state only."""
    seq = list(seq)
    if len(seq) < 64:
        return [fn(x) for x in seq]
    step = (len(seq) + 8 * workers - 1) // (8 * workers)
    parts = [seq[i : i + step] for i in range(0, len(seq), step)]
    with ThreadPoolExecutor(workers) as ex:
        return [y for part in ex.map(lambda p: [fn(x) for x in p], parts) for y in part]


def rng_at(oracle, seed, skip):
    r = oracle.rng_from_u64(seed)
    for _ in range(skip):
        oracle.rng_fill64(r)
    return r


def key_set(oracle, shares_n, threshold, seed):
    """A Shamir key set as in test_threshold_tally_end_to_end: (shared key, secret shares, participant keys)."""
    rnd = random.Random(seed)
    coeffs = [rnd.randrange(L) for _ in range(threshold)]
    f = lambda x: sum(c * pow(x, k, L) for k, c in enumerate(coeffs)) % L
    sks = [f(i + 1) for i in range(shares_n)]
    return oracle.point_mul_generator(sc(coeffs[0])), sks, [oracle.point_mul_generator(sc(s)) for s in sks]


class Kind:
    """One proof kind: how the GPU makes and checks its items, how the oracle does, and where the items' parts lie."""

    def __init__(self, oracle, pk, kind, bound=0, n_values=0, share=None):
        self.o, self.pk, self.kind, self.bound, self.n_values, self.share = oracle, pk, kind, bound, n_values, share
        self.k = oracle.PublicKey(pk)
        if kind == ZERO:
            self.name, self.size, self.n_points = "zero", 128, 2
        elif kind == BOOL:
            self.name, self.size, self.n_points = "bool", 160, 2
        elif kind == RANGE:
            self.pr = oracle.PreparedRange(bound)
            self.name, self.size, self.n_points = f"range{bound}", 64 + self.pr.proof_size, 2 * len(self.pr.rings)
        elif kind == SUMSQ:
            self.name, self.size, self.n_points = f"sumsq{n_values}", 64 * (n_values + 1) + 32 * (2 * n_values + 2), 2 * n_values + 2
        else:
            # share = (shares, threshold, shared key, index, secret share, participant key)
            self.name, self.size, self.n_points = f"share{share[3]}of{share[0]}", 128, 2
        self.n_items = self.size // 32             # points, then the challenge, then the responses

    def verifier(self, eg, ctx):
        if self.kind == SUMSQ:
            return eg.SumOfSquaresVerifier(ctx, self.pk, self.n_values, b"test")
        if self.kind == SHARE:
            n, t, shared, idx, _, part = self.share
            return eg.DecryptionShareVerifier(ctx, shared, n, t, idx, part)
        return eg.PublicKeyVerifier(ctx, self.pk, self.kind, self.bound)

    def gpu_prove(self, ver, seed, first, inputs, skip=0):
        """inputs: the number of items (zero), values (bool, range), value lists (sumsq), random elements as bytes (share)."""
        if self.kind == SHARE:
            items, ok = ver.prove(sc(self.share[4]), seed, first, inputs, rng_skip=skip)
            assert set(ok) <= {1}
            return items
        return ver.prove(seed, first, inputs, rng_skip=skip)

    def oracle_prove(self, seed, inp, skip=0):
        r = rng_at(self.o, seed, skip)
        if self.kind == ZERO:
            return self.k.encrypt_zero(r)
        if self.kind == BOOL:
            return self.k.encrypt_bool(bool(inp), r)
        if self.kind == RANGE:
            return self.k.encrypt_range(self.pr, inp, r)
        if self.kind == SUMSQ:
            cts, proof = self.k.sumsq_snapshot(list(inp), r)        # the sum's ciphertext comes first there, last in the item
            return cts[64:] + cts[:64] + proof
        n, t, shared, idx, sk, _ = self.share
        return inp + self.o.decryption_share_new(sc(sk), inp, n, t, shared, idx, r)

    def oracle_verify(self, item):
        if self.kind == ZERO:
            return self.k.verify_zero(item)
        if self.kind == BOOL:
            return self.k.verify_bool(item)
        if self.kind == RANGE:
            return self.k.verify_range(self.pr, item)
        if self.kind == SUMSQ:
            n = self.n_values
            return self.k.verify_sumsq(item[: 64 * n], item[64 * n : 64 * n + 64], item[64 * n + 64 :], b"test")
        n, t, shared, idx, _, part = self.share
        return self.o.decryption_share_verify(part, n, t, shared, idx, item)

    def split(self, packed):
        assert len(packed) % self.size == 0
        return [packed[i : i + self.size] for i in range(0, len(packed), self.size)]


def random_inputs(kd, rnd, n, grp=None):
    if kd.kind == ZERO:
        return n
    if kd.kind == BOOL:
        return [rnd.randrange(2) for _ in range(n)]
    if kd.kind == RANGE:
        return [0, 1, kd.bound - 1] + [rnd.randrange(kd.bound) for _ in range(n - 3)]
    if kd.kind == SUMSQ:
        return [[0] * kd.n_values] + [[rnd.choice((0, 0, 1, 2, 7, 1000, 2**28)) if rnd.random() < 0.5 else rnd.randrange(2**20)
                                       for _ in range(kd.n_values)] for _ in range(n - 1)]
    return grp.mul_generator(b"".join(sc(rnd.randrange(1, L)) for _ in range(n)))        # random elements R = [k]G


def input_at(kd, inputs, i):
    return None if kd.kind == ZERO else (inputs[32 * i : 32 * i + 32] if kd.kind == SHARE else inputs[i])


def inputs_slice(kd, inputs, a, b):
    return b - a if kd.kind == ZERO else (inputs[32 * a : 32 * b] if kd.kind == SHARE else inputs[a:b])


@pytest.fixture(scope="module")
def share_sets(oracle):
    """Two participants each of a 2-of-3 and a 7-of-10 key set."""
    out = []
    for n, t, seed in ((3, 2, 23), (10, 7, 710)):
        shared, sks, parts = key_set(oracle, n, t, seed)
        for idx in (0, n - 1):
            out.append((n, t, shared, idx, sks[idx], parts[idx]))
    return out


# ------------------------------------------------------------------ 1. snapshots
def test_provers_reproduce_the_reference_snapshots(eg, ctx, oracle, golden, pk):
    """tests/snapshots.rs with seed 12345 and the keypair draw skipped (rng_skip = 1): `zero-encryption`, `bool-encryption` (true),
    `range-encryption` (bound 100, value 42) and the `sum-sq-proof` proof for [1, 3, 3, 7, 5] under the label "test", whose
    ciphertexts the snapshot does not hold: they are the oracle's."""
    seed = golden["seed"]
    z = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.ZERO)
    b = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.BOOL)
    g = golden["range-encryption"]["params"]
    r = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.RANGE, g["upper_bound"])
    vals = golden["sum-sq-proof"]["params"]["values"]
    s = eg.SumOfSquaresVerifier(ctx, pk, len(vals), golden["sum-sq-proof"]["params"]["label"].encode())
    try:
        got = z.prove(seed, 0, 1, rng_skip=1)
        assert got.hex() == golden["zero-encryption"]["packed"] and z.verify_batch(got) == [0]
        got = b.prove(seed, 0, [golden["bool-encryption"]["params"]["value"]], rng_skip=1)
        assert got.hex() == golden["bool-encryption"]["packed"] and b.verify_batch(got) == [0]
        got = r.prove(seed, 0, [g["value"]], rng_skip=1)
        assert got.hex() == golden["range-encryption"]["packed"] and r.verify_batch(got) == [0]
        got = s.prove(seed, 0, [vals], rng_skip=1)
        n = len(vals)
        assert got[64 * (n + 1) :].hex() == golden["sum-sq-proof"]["packed"] and s.verify_batch(got) == [0]
        cts, proof = oracle.PublicKey(pk).sumsq_snapshot(vals, oracle.keypair_from_seed(seed)[2])
        assert got == cts[64:] + cts[:64] + proof
        # the snapshot is item 5 of a batch as well as item 0 of its own
        assert z.prove(seed - 5, 0, 7, rng_skip=1)[5 * 128 : 6 * 128].hex() == golden["zero-encryption"]["packed"]
        assert s.prove(seed - 5, 2, [[0] * n] * 3 + [vals], rng_skip=1)[3 * s.item_size :] == got
    finally:
        for v in (z, b, r, s):
            v.close()


# ------------------------------------------------------------------ 2. byte parity with the oracle's provers
def parity(eg, ctx, grp, kd, n, seed):
    """n items over rng_skip 0, 1 and 5 against the oracle item by item; `first` != 0 against first = 0; host against device entry."""
    import torch

    rnd = random.Random(seed)
    ver = kd.verifier(eg, ctx)
    try:
        assert ver.item_size == kd.size
        per = n // 3
        for skip in (0, 1, 5):
            inputs = random_inputs(kd, rnd, per, grp)
            base = seed * 1000 + skip
            its = kd.split(kd.gpu_prove(ver, base, 0, inputs, skip))
            want = pmap(lambda i: kd.oracle_prove(base + i, input_at(kd, inputs, i), skip), range(per))
            bad = [i for i in range(per) if its[i] != want[i]]
            assert not bad, (kd.name, skip, len(bad), bad[:5])
            assert ver.verify_batch(b"".join(its)) == [0] * per
            # the same items as the tail of a call that starts elsewhere
            cut = per // 3 + 1
            tail = kd.gpu_prove(ver, base, cut, inputs_slice(kd, inputs, cut, per), skip)
            assert tail == b"".join(its[cut:]), (kd.name, skip)
            assert kd.gpu_prove(ver, base + cut, 0, inputs_slice(kd, inputs, cut, per), skip) == tail
        # device entry: same bytes
        d_items = torch.zeros(per * kd.size, dtype=torch.uint8, device="cuda")
        if kd.kind == SHARE:
            d_in = torch.frombuffer(bytearray(inputs), dtype=torch.uint8).cuda()
            d_ok = torch.zeros(per, dtype=torch.uint8, device="cuda")
            ver.prove_device(sc(kd.share[4]), base, 0, per, d_in.data_ptr(), d_items.data_ptr(), d_ok.data_ptr(), rng_skip=5)
            ver.ctx.synchronize()
            assert d_ok.cpu().tolist() == [1] * per
        else:
            flat = [] if kd.kind == ZERO else ([x for row in inputs for x in row] if kd.kind == SUMSQ else [int(v) for v in inputs])
            d_in = torch.tensor(flat, dtype=torch.int64, device="cuda") if flat else None
            s = torch.cuda.Stream()
            ver.prove_device(base, 0, per, d_in.data_ptr() if flat else 0, d_items.data_ptr(), rng_skip=5, stream=s.cuda_stream)
            s.synchronize()
        assert bytes(d_items.cpu().numpy().tobytes()) == b"".join(its), kd.name
    finally:
        ver.close()


def test_zero_prover_matches_the_oracle(eg, ctx, oracle, pk):
    parity(eg, ctx, None, Kind(oracle, pk, ZERO), 2100, 1)


def test_bool_prover_matches_the_oracle(eg, ctx, oracle, pk):
    parity(eg, ctx, None, Kind(oracle, pk, BOOL), 2100, 2)         # both values, by the coin of random_inputs


@pytest.mark.parametrize("bound", [2, 5, 100, 1000, 10**6])
def test_range_prover_matches_the_oracle(eg, ctx, oracle, pk, bound):
    parity(eg, ctx, None, Kind(oracle, pk, RANGE, bound=bound), 420, 3 + bound)          # 2 100 seeds over the bounds; 0, 1, bound - 1 in each


@pytest.mark.parametrize("n_values", [1, 2, 5, 16])
def test_sumsq_prover_matches_the_oracle(eg, ctx, oracle, pk, n_values):
    parity(eg, ctx, None, Kind(oracle, pk, SUMSQ, n_values=n_values), 540, 40 + n_values)


def test_share_prover_matches_the_oracle(eg, ctx, oracle, pk, share_sets):
    grp = eg.Ristretto(ctx)
    for share in share_sets:
        parity(eg, ctx, grp, Kind(oracle, pk, SHARE, share=share), 540, 50 + share[0] + share[3])


# ------------------------------------------------------------------ 3. the verifiers at size
N_SIZE = 100_037            # not a multiple of 64; with EG_CHUNK = 30 011 it spans four ragged chunks
CHUNK = 30_011
_at_size = {}


def tamper(kd, rnd, item, mode):
    """mode 0: a flipped bit in a ciphertext (or R / dh) element; 1: in the challenge; 2: in a response; 3: a non-canonical scalar."""
    t = bytearray(item)
    n_pts, n_items = kd.n_points, kd.n_items
    if mode == 0:
        pos = 256 * rnd.randrange(n_pts) + rnd.randrange(256)
    elif mode == 1:
        pos = 256 * n_pts + rnd.randrange(252)
    elif mode == 2:
        pos = 256 * rnd.randrange(n_pts + 1, n_items) + rnd.randrange(252)
    else:
        k = rnd.randrange(n_pts, n_items)
        t[32 * k : 32 * k + 32] = rnd.choice((L, L + 1, 2**256 - 1, L + rnd.getrandbits(200))).to_bytes(32, "little")
        return bytes(t)
    t[pos // 8] ^= 1 << (pos % 8)
    return bytes(t)


def at_size_case(eg, oracle, pk, name, share_sets):
    """The 100 037 GPU-made items of one kind, a tenth tampered, and the oracle's verdicts on every tampered item and on `extra`
    untampered ones (all of them where an item costs the oracle a third of a millisecond) - made once, used with both table widths."""
    if name in _at_size:
        return _at_size[name]
    kd = {"zero": lambda: Kind(oracle, pk, ZERO), "bool": lambda: Kind(oracle, pk, BOOL),
          "range": lambda: Kind(oracle, pk, RANGE, bound=100), "sumsq": lambda: Kind(oracle, pk, SUMSQ, n_values=5),
          "share": lambda: Kind(oracle, pk, SHARE, share=share_sets[3])}[name]()
    c = eg.Context(0)
    try:
        ver = kd.verifier(eg, c)
        rnd = random.Random(sum(map(ord, name)))
        inputs = random_inputs(kd, rnd, N_SIZE, eg.Ristretto(c))
        its = kd.split(kd.gpu_prove(ver, 880000, 0, inputs))
        ver.close()
    finally:
        c.close()
    assert len(its) == N_SIZE
    fixed = [0, 63, 64, N_SIZE - 1, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK]       # lanes 0 / 63 / 64 / last, and the chunk seams
    rest = rnd.sample([i for i in range(N_SIZE) if i not in set(fixed)], N_SIZE // 10 - len(fixed))
    tampered = fixed + rest
    for k, i in enumerate(tampered):
        its[i] = tamper(kd, rnd, its[i], k % 4)
    hit = set(tampered)
    clean = [i for i in range(N_SIZE) if i not in hit]
    extra = clean if name in ("zero", "bool", "share") else rnd.sample(clean, 2 * len(tampered))
    checked = sorted(tampered + extra)
    want = dict(zip(checked, pmap(lambda i: kd.oracle_verify(its[i]), checked)))
    _at_size[name] = (kd, b"".join(its), tampered, want)
    return _at_size[name]


@pytest.mark.parametrize("big_bits", [24, 0])
@pytest.mark.parametrize("name", ["zero", "bool", "range", "sumsq", "share"])
def test_verifier_at_size_on_gpu_made_items(eg, oracle, pk, share_sets, monkeypatch, name, big_bits):
    kd, packed, tampered, want = at_size_case(eg, oracle, pk, name, share_sets)
    monkeypatch.setenv("EG_COMB_BIG_MIN", "1")
    monkeypatch.setenv("EG_COMB_BIG_BITS", str(big_bits))
    monkeypatch.setenv("EG_CHUNK", str(CHUNK))
    c = eg.Context(0)
    try:
        ver = kd.verifier(eg, c)
        got = ver.verify_batch(packed)
        assert c.comb_table_bits() == (20, big_bits)
        ver.close()
    finally:
        c.close()
    assert len(got) == N_SIZE
    bad = [i for i in want if got[i] != want[i]]
    assert not bad, (name, len(bad), [(i, got[i], want[i]) for i in bad[:10]])
    hit = set(tampered)
    stray = [i for i in range(N_SIZE) if i not in hit and got[i] != 0]        # NO untampered item is left out of this check
    assert not stray, (name, len(stray), stray[:10])
    assert all(got[i] != 0 for i in tampered)                                 # the fixed lanes and chunk seams among them
    kinds = {s & 0xFF for s in got}
    assert {0, eg.BAD_SCALAR, eg.BAD_POINT} < kinds and len(kinds) == 4, kinds       # plus the kind's own challenge mismatch
    assert {s >> 8 for s in got if s & 0xFF == eg.BAD_SCALAR} <= set(range(kd.n_points, kd.n_items))
    assert {s >> 8 for s in got if s & 0xFF == eg.BAD_POINT} == set(range(kd.n_points))


# ------------------------------------------------------------------ 4. bad inputs
def test_share_prover_marks_invalid_random_elements(eg, ctx, oracle, pk, share_sets):
    import torch

    kd = Kind(oracle, pk, SHARE, share=share_sets[1])
    ver = kd.verifier(eg, ctx)
    try:
        n = 64 * 5 + 3
        rnd = random.Random(9)
        good = random_inputs(kd, rnd, n, eg.Ristretto(ctx))
        bad_at = {0: BAD_POINT_BYTES, 63: b"\xff" * 32, 64: (2**255 - 19).to_bytes(32, "little"), 200: b"\x02" + bytes(30) + b"\x80",
                  n - 1: BAD_POINT_BYTES}
        rs = [bad_at.get(i, good[32 * i : 32 * i + 32]) for i in range(n)]
        assert all(oracle.point_roundtrip(b) is None for b in bad_at.values())
        items, ok = ver.prove(sc(kd.share[4]), 31, 0, b"".join(rs))
        its = kd.split(items)
        marks = [0 if i in bad_at else 1 for i in range(n)]
        assert list(ok) == marks
        for i in range(n):
            assert its[i] == (bytes(128) if i in bad_at else kd.oracle_prove(31 + i, rs[i])), i
        # the identity is an element: its share is the identity, and the proof verifies
        items, ok = ver.prove(sc(kd.share[4]), 32, 0, bytes(32))
        assert ok == b"\x01" and items[:64] == bytes(64) and items == kd.oracle_prove(32, bytes(32))
        assert ver.verify_batch(items) == [0] == [kd.oracle_verify(items)]
        # a wrong share is not refused: its items do not verify (log_equality.rs:111-113)
        wrong, ok = ver.prove(sc(kd.share[4] + 1), 33, 0, good[:96])
        assert set(ok) == {1} and ver.verify_batch(wrong) == [eg.SUM_CHALLENGE] * 3
        # device entry: same marks
        d_in = torch.frombuffer(bytearray(b"".join(rs)), dtype=torch.uint8).cuda()
        d_items = torch.full((n * 128,), 7, dtype=torch.uint8, device="cuda")
        d_ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        ver.prove_device(sc(kd.share[4]), 31, 0, n, d_in.data_ptr(), d_items.data_ptr(), d_ok.data_ptr())
        ver.ctx.synchronize()
        assert bytes(d_items.cpu().numpy().tobytes()) == b"".join(its) and d_ok.cpu().tolist() == marks
    finally:
        ver.close()


def test_refused_arguments(eg, ctx, oracle, pk, share_sets):
    lib = eg._load()
    n, t, shared, idx, sk, part = share_sets[0]
    z = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.ZERO)
    b = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.BOOL)
    r = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.RANGE, 100)
    s = eg.SumOfSquaresVerifier(ctx, pk, 2, b"test")
    d = eg.DecryptionShareVerifier(ctx, shared, n, t, idx, part)
    ce = eg.CommitmentEquivalenceVerifier(ctx, pk, oracle.point_mul_generator(sc(5)), b"test")
    try:
        assert [lib.eg_proof_prove_input_size(v._h) for v in (z, b, r, s, d, ce)] == [0, 8, 8, 16, 0, 0]
        vals = (C.c_uint64 * 4)(1, 0, 1, 0)
        buf = C.create_string_buffer(4 * 672)
        okb = C.create_string_buffer(4)
        host, dev = lib.eg_proof_prove_batch, lib.eg_proof_prove_batch_device
        # the wrong kind for an entry
        assert host(d._h, 1, 0, 2, 0, vals, buf) == BAD_ARG and host(ce._h, 1, 0, 2, 0, vals, buf) == BAD_ARG
        assert dev(d._h, 1, 0, 2, 0, None, None, None) == BAD_ARG and dev(ce._h, 1, 0, 2, 0, None, None, None) == BAD_ARG
        for v in (z, b, r, s, ce):
            assert lib.eg_share_prove_batch(v._h, sc(sk), 1, 0, 1, 0, part, buf, okb) == BAD_ARG
            assert lib.eg_share_prove_batch_device(v._h, sc(sk), 1, 0, 1, 0, None, None, None, None) == BAD_ARG
        # a NULL where a buffer is required
        assert host(None, 1, 0, 2, 0, vals, buf) == BAD_ARG and dev(None, 1, 0, 2, 0, None, None, None) == BAD_ARG
        for v in (b, r, s):
            assert host(v._h, 1, 0, 2, 0, None, buf) == BAD_ARG and host(v._h, 1, 0, 2, 0, vals, None) == BAD_ARG
            assert dev(v._h, 1, 0, 2, 0, None, None, None) == BAD_ARG
        assert host(z._h, 1, 0, 2, 0, None, None) == BAD_ARG and dev(z._h, 1, 0, 2, 0, None, None, None) == BAD_ARG
        assert host(z._h, 1, 0, 2, 0, None, buf) == 0                                    # zero takes no input
        assert lib.eg_share_prove_batch(d._h, None, 1, 0, 1, 0, part, buf, okb) == BAD_ARG
        assert lib.eg_share_prove_batch(d._h, sc(sk), 1, 0, 1, 0, None, buf, okb) == BAD_ARG
        assert lib.eg_share_prove_batch(d._h, sc(sk), 1, 0, 1, 0, part, None, okb) == BAD_ARG
        assert lib.eg_share_prove_batch(d._h, sc(sk), 1, 0, 1, 0, part, buf, None) == BAD_ARG
        assert lib.eg_share_prove_batch_device(d._h, sc(sk), 1, 0, 1, 0, None, None, None, None) == BAD_ARG
        # nothing to do
        assert host(b._h, 1, 0, 0, 0, None, None) == 0 and lib.eg_share_prove_batch(d._h, sc(sk), 1, 0, 0, 0, None, None, None) == 0
        # the host forms' value checks
        for v, rows in ((b, [0, 1, 2]), (b, [2**64 - 1]), (r, [0, 100]), (r, [99, 2**63]), (s, [[1, 1], [2**32, 0]]),
                        (s, [[2**32 - 1, 92682]]), (s, [[2**64 - 1, 2**64 - 1]])):
            with pytest.raises(eg.EgError):
                v.prove(1, 0, rows)
        for bad_share in (L, L + 1, 2**256 - 1):
            with pytest.raises(eg.EgError, match="canonical"):
                d.prove(bad_share.to_bytes(32, "little"), 1, 0, part)
        with pytest.raises(ValueError):
            s.prove(1, 0, [[1, 2, 3]])
        # ... and the edge values pass and verify
        assert b.verify_batch(b.prove(1, 0, [1, 0, True, False])) == [0] * 4
        assert r.verify_batch(r.prove(1, 0, [99, 0])) == [0, 0]
        assert s.verify_batch(s.prove(1, 0, [[2**32 - 1, 92681], [0, 0]])) == [0, 0]
        items, ok = d.prove(sc(L - 1), 1, 0, part)                                        # the largest canonical scalar is a share
        assert ok == b"\x01" and items[32:64] == oracle.point_multi_mul(sc(L - 1), part)
    finally:
        for v in (z, b, r, s, d, ce):
            v.close()


# ------------------------------------------------------------------ 5. neighbours
def test_proving_leaves_the_verifiers_and_the_ballot_generators_alone(eg, oracle, golden, pk, share_sets):
    c = eg.Context(0)
    try:
        k = oracle.PublicKey(pk)
        rs = oracle.rng_from_u64(404)
        pr = oracle.PreparedRange(100)
        zs = [bytearray(k.encrypt_zero(rs)) for _ in range(90)]
        gs = [bytearray(k.encrypt_range(pr, (7 * i) % 100, rs)) for i in range(90)]
        for i in range(1, 90, 4):
            zs[i][(i * 7) % 128] ^= 1
            gs[i][(i * 11) % 672] ^= 2
        zb, gb = b"".join(map(bytes, zs)), b"".join(map(bytes, gs))
        z = eg.PublicKeyVerifier(c, pk, eg.PublicKeyVerifier.ZERO)
        r = eg.PublicKeyVerifier(c, pk, eg.PublicKeyVerifier.RANGE, 100)
        before = (z.verify_batch(zb), r.verify_batch(gb))
        assert before == ([k.verify_zero(bytes(x)) for x in zs], [k.verify_range(pr, bytes(x)) for x in gs])
        assert all(0 in v and any(v) for v in before)
        # two kinds of one context prove in turn, small and large batches (the range prover's workspace grows in between)
        for n in (3, 5000, 7):
            zi = z.prove(5, 0, n)
            ri = r.prove(5, 0, [(13 * i) % 100 for i in range(n)])
            assert z.verify_batch(zi) == [0] * n and r.verify_batch(ri) == [0] * n
            assert ri[:672] == k.encrypt_range(pr, 0, oracle.rng_from_u64(5)) and zi[:128] == k.encrypt_zero(oracle.rng_from_u64(5))
            assert (z.verify_batch(zb), r.verify_batch(gb)) == before
        # the ballot generators, called anew beside them, still reproduce the reference's snapshots
        g = golden["encrypted-choice"]
        p = eg.ChoiceParams.single_choice(c, pk, g["params"]["options"])
        assert p.encrypt_selected(golden["seed"], 0, [1 << g["params"]["choice"]], rng_skip=1).hex() == g["packed"]
        g = golden["qv-ballot"]
        q = eg.QuadraticVotingParams(c, pk, g["params"]["options"], g["params"]["credits"])
        assert q.encrypt_votes(golden["seed"], 0, [g["params"]["votes"]], rng_skip=1).hex() == g["packed"]
        n = 300                                                                          # and a batch of QV ballots against the oracle
        import torch

        buf = torch.zeros(n * q.ballot_size, dtype=torch.uint8, device="cuda")
        q.encrypt_batch_device(77, 0, n, buf.data_ptr())
        c.synchronize()
        assert bytes(buf.cpu().numpy().tobytes()) == oracle.QvParams(pk, g["params"]["options"], g["params"]["credits"]).generate_batch(77, 0, n)
        assert (z.verify_batch(zb), r.verify_batch(gb)) == before
        for o in (z, r, p, q):
            o.close()
    finally:
        c.close()
