"""GPU parity tests: the HIP path (through the C ABI, include/eg_hip.h) against the CPU oracle on the same
seeded inputs, against the committed golden fixtures, and through size-independent properties.
Bit-exact everywhere: this path is integer/byte work."""
import base64
import random

import pytest

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493
P = 2**255 - 19


def unb64(s):
    return base64.urlsafe_b64decode(s + "=" * (-len(s) % 4))


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
def grp(eg, ctx):
    return eg.Ristretto(ctx)


@pytest.fixture(scope="module")
def pk(golden):
    return unb64(golden["public_key_b64"])


def sc(x):
    return (x % L).to_bytes(32, "little")


# ------------------------------------------------------------------ primitive tier
def test_scalars(grp, oracle):
    rnd = random.Random(1)
    wides = [rnd.getrandbits(512).to_bytes(64, "little") for _ in range(500)] + [b"\xff" * 64, b"\0" * 64]
    got = grp.scalar_from_random_bytes(b"".join(wides))
    for i, w in enumerate(wides):
        assert got[32 * i : 32 * i + 32] == oracle.sc_from_wide(w)
    vals = [0, 1, L - 1, 2**252] + [rnd.randrange(L) for _ in range(200)]
    a = b"".join(sc(v) for v in vals)
    b = b"".join(sc(rnd.randrange(L)) for _ in vals)
    c = b"".join(sc(rnd.randrange(L)) for _ in vals)
    got = grp.scalar_muladd(a, b, c)
    neg = grp.scalar_neg(a)
    for i, v in enumerate(vals):
        bi = int.from_bytes(b[32 * i : 32 * i + 32], "little")
        ci = int.from_bytes(c[32 * i : 32 * i + 32], "little")
        assert int.from_bytes(got[32 * i : 32 * i + 32], "little") == (v * bi + ci) % L
        assert int.from_bytes(neg[32 * i : 32 * i + 32], "little") == (-v) % L
    cand = [sc(0), sc(L - 1), L.to_bytes(32, "little"), (L + 1).to_bytes(32, "little"), b"\xff" * 32]
    assert list(grp.deserialize_scalar_ok(b"".join(cand))) == [1, 1, 0, 0, 0]
    inv = grp.invert_scalars(a)   # ScalarOps::invert_scalars; known answers from Fermat (l is prime)
    for i, v in enumerate(vals):
        assert int.from_bytes(inv[32 * i : 32 * i + 32], "little") == pow(v, L - 2, L), i


def test_element_codec(grp, oracle):
    rnd = random.Random(2)
    valid = [oracle.point_mul_generator(sc(rnd.randrange(L))) for _ in range(64)] + [b"\0" * 32, oracle.const_bytes(4)]
    junk = [rnd.getrandbits(255).to_bytes(32, "little") for _ in range(400)] + [b"\xff" * 32, P.to_bytes(32, "little"), (1).to_bytes(32, "little")]
    items = valid + junk
    out, ok = grp.element_roundtrip(b"".join(items))
    for i, e in enumerate(items):
        want = oracle.point_roundtrip(e)
        assert bool(ok[i]) == (want is not None), i
        if want is not None:
            assert out[32 * i : 32 * i + 32] == want == e
    flags, ok2 = grp.is_identity(b"".join(items))
    assert list(ok2) == list(ok)
    assert [i for i, f in enumerate(flags) if f] == [items.index(b"\0" * 32)]
    a, b = valid[:32], valid[32:64]
    neg, _ = grp.element_neg(b"".join(a))
    back, _ = grp.element_add(b"".join(a), neg)
    assert back == b"\0" * (32 * 32)
    s, ok = grp.element_add(b"".join(a), b"".join(b))
    d, _ = grp.element_add(b"".join(a), b"".join(b), subtract=True)
    for i in range(32):
        assert s[32 * i : 32 * i + 32] == oracle.point_add(a[i], b[i])
        assert d[32 * i : 32 * i + 32] == oracle.point_add(a[i], b[i], sub=True)


def test_scalar_multiplication(grp, oracle):
    rnd = random.Random(3)
    n = 300
    edge = [0, 1, 8, 15, 16, L - 1, 2**252, 0x0888888888888888888888888888888888888888888888888888888888888888, 2**252 + 2**128]
    ks = [edge[i % len(edge)] if i < 2 * len(edge) else rnd.randrange(L) for i in range(n)]
    rs = [rnd.randrange(L) if i % 7 else edge[i % len(edge)] for i in range(n)]
    pts = [oracle.point_mul_generator(sc(rnd.randrange(L))) if i % 11 else b"\0" * 32 for i in range(n)]
    got = grp.mul_generator(b"".join(sc(k) for k in ks))
    for i in range(n):
        assert got[32 * i : 32 * i + 32] == oracle.point_mul_generator(sc(ks[i]))
    got, ok = grp.vartime_double_mul_generator(b"".join(sc(k) for k in ks), b"".join(pts), b"".join(sc(r) for r in rs))
    assert set(ok) == {1}
    for i in range(n):
        assert got[32 * i : 32 * i + 32] == oracle.point_double_mul_generator(sc(ks[i]), pts[i], sc(rs[i])), i
    for terms in (1, 2, 3, 7):
        m = 40
        scal = [[sc(rnd.randrange(L)) for _ in range(terms)] for _ in range(m)]
        pp = [[rnd.choice(pts) for _ in range(terms)] for _ in range(m)]
        got, ok = grp.vartime_multi_mul(terms, b"".join(b"".join(x) for x in scal), b"".join(b"".join(x) for x in pp))
        for i in range(m):
            assert got[32 * i : 32 * i + 32] == oracle.point_multi_mul(b"".join(scal[i]), b"".join(pp[i])), (terms, i)
    # invalid input points are flagged
    got, ok = grp.vartime_double_mul_generator(sc(5), b"\xff" * 32, sc(7))
    assert ok == b"\0"


def _check_prepared_points(eg, ctx, grp, m, terms, ds, dp, dr, want_out):
    """eg_points_prepare_device + eg_vartime_multi_mul_prepared_batch_device (ristretto.rs:139-145 takes decoded Elements): the same
    operands, decoded once into prepared points, give the same encodings as the entry that decodes per term."""
    import torch

    n_pts = m * terms
    assert eg.prepared_point_size() == 96
    prep = torch.zeros(n_pts * 96, dtype=torch.uint8, device="cuda")
    pok = torch.zeros(n_pts, dtype=torch.uint8, device="cuda")
    grp.prepare_points_device(n_pts, dp.data_ptr(), prep.data_ptr(), d_ok=pok.data_ptr())
    do = torch.zeros(32 * m, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(max(grp.msm_scratch_bytes(m, terms), 16), dtype=torch.uint8, device="cuda")
    grp.vartime_multi_mul_prepared_device(m, terms, ds.data_ptr(), prep.data_ptr(), do.data_ptr(), d_r=dr.data_ptr(), d_scratch=scratch.data_ptr())
    ctx.synchronize()
    assert int(pok.min()) == 1
    assert bytes(do.cpu().numpy()) == want_out, (m, terms)


def test_multi_scalar_mul_any_size(eg, ctx, grp, oracle):
    """Group::vartime_multi_mul for every size class of the kernel (ristretto.rs:139-145; dalek: Straus / Pippenger): one chunk (<= 8
    terms on one doubling chain), several chunks reduced with wave shuffles (9, 16, 255, 256 terms) and one 65 536-term product;
    identity points, zero and edge scalars inside; an undecodable point anywhere flags the problem.  Host and device entry points agree."""
    import torch

    import os

    rnd = random.Random(77)
    pool = [oracle.point_mul_generator(sc(rnd.randrange(L))) for _ in range(40)] + [b"\0" * 32]
    edge = [0, 1, L - 1, 2**252, 8, 0x0888888888888888888888888888888888888888888888888888888888888888]
    # a call with few terms in all is cut into single-term chunks so that it covers the chip; EG_MSM_LANES=1 keeps the chunks of 8
    # terms (one shared doubling chain each) that large batches get: both cuts are checked for every size
    # (the knob is read once, by eg_init: a second context carries it)
    os.environ["EG_MSM_LANES"] = "1"
    ctx1 = eg.Context(0)
    os.environ.pop("EG_MSM_LANES", None)
    default = (ctx, grp)
    for lanes, terms, m in [(l, t, k) for l in ("1", None) for t, k in ((8, 5), (9, 4), (16, 4), (255, 2), (256, 2), (65536, 1))]:
        ctx, grp = default if lanes is None else (ctx1, eg.Ristretto(ctx1))
        scal = [[sc(edge[(i + t) % len(edge)]) if t % 5 == 0 else sc(rnd.randrange(L)) for t in range(terms)] for i in range(m)]
        pp = [[pool[rnd.randrange(len(pool))] for _ in range(terms)] for _ in range(m)]
        sb, pb = b"".join(b"".join(x) for x in scal), b"".join(b"".join(x) for x in pp)
        got, ok = grp.vartime_multi_mul(terms, sb, pb)
        assert set(ok) == {1}
        for i in range(m):
            assert got[32 * i : 32 * i + 32] == oracle.point_multi_mul(b"".join(scal[i]), b"".join(pp[i])), (terms, i)
        # device entry point with a generator term: [r]G + sum
        r = b"".join(sc(rnd.randrange(L)) for _ in range(m))
        ds = torch.frombuffer(bytearray(sb), dtype=torch.uint8).cuda()
        dp = torch.frombuffer(bytearray(pb), dtype=torch.uint8).cuda()
        dr = torch.frombuffer(bytearray(r), dtype=torch.uint8).cuda()
        do = torch.zeros(32 * m, dtype=torch.uint8, device="cuda")
        dok = torch.zeros(m, dtype=torch.uint8, device="cuda")
        scratch = torch.zeros(max(grp.msm_scratch_bytes(m, terms), 16), dtype=torch.uint8, device="cuda")
        grp.vartime_multi_mul_device(m, terms, ds.data_ptr(), dp.data_ptr(), do.data_ptr(), d_r=dr.data_ptr(), d_scratch=scratch.data_ptr(),
                                     d_ok=dok.data_ptr())
        ctx.synchronize()
        out = bytes(do.cpu().numpy())
        for i in range(m):
            want = oracle.point_add(got[32 * i : 32 * i + 32], oracle.point_mul_generator(r[32 * i : 32 * i + 32]))
            assert out[32 * i : 32 * i + 32] == want, (terms, i)
        assert dok.cpu().tolist() == [1] * m
        _check_prepared_points(eg, ctx, grp, m, terms, ds, dp, dr, out)
        if terms in (9, 256):          # one undecodable point in the last chunk of problem 1
            bad = bytearray(pb)
            bad[(1 * terms + terms - 1) * 32 : (1 * terms + terms) * 32] = b"\xff" * 32
            _, ok = grp.vartime_multi_mul(terms, sb, bytes(bad))
            assert list(ok) == [1, 0] + [1] * (m - 2)
    ctx1.close()
    assert grp.vartime_multi_mul(0, b"", b"") == (b"", b"")


def test_comb_tables_selfcheck_and_digit_corners(eg, ctx, grp, oracle):
    """The fixed-base comb tables are built run by run with a batched inversion (k_build_fixed_table): sampled entries and the corners
    of windows and runs equal an entry-by-entry recomputation, for the table built at start-up and for the wide one; scalars whose
    comb digits sit on the corners of the 64-entry runs and on the extreme digits give the oracle's products."""
    assert ctx.selfcheck_generator_table(False, 30000, 7) == 0
    assert ctx.selfcheck_generator_table(True, 30000, 8) == 0
    digits = [1, 2, 63, 64, 65, 127, 128, 129, 2**19 - 1, 2**19, 2**19 + 1, 2**20 - 1, 2**20 - 64, 2**20 - 65]
    ks = []
    for w in range(13):
        for d in digits:
            ks.append((d << (20 * w)) % L)
    ks += [sum(d << (20 * w) for w, d in enumerate([2**19] * 12)) % L, sum((2**20 - 1) << (20 * w) for w in range(12)) % L]
    got = grp.mul_generator(b"".join(sc(k) for k in ks))
    for i, k in enumerate(ks):
        assert got[32 * i : 32 * i + 32] == oracle.point_mul_generator(sc(k)), hex(k)


@pytest.mark.parametrize("big_bits", [24, 22, 0])
def test_wide_comb_tables_give_the_same_verdicts(eg, oracle, pk, monkeypatch, big_bits):
    """An engine that has verified EG_COMB_BIG_MIN items switches to the wide comb tables (24-bit windows, 11 instead of 13 additions
    per comb).  Forced from the first ballot here, also with another width and switched off: verdicts and tally are the oracle's."""
    monkeypatch.setenv("EG_COMB_BIG_MIN", "1")
    monkeypatch.setenv("EG_COMB_BIG_BITS", str(big_bits))
    c = eg.Context(0)
    try:
        rnd = random.Random(11)
        op = oracle.ChoiceParams(pk, 5, True)
        ballots = _tamper_choice(op.generate_batch(78, 0, 200), op.ballot_size, oracle, rnd)
        want = op.verify_batch(ballots)
        p = eg.ChoiceParams(c, pk, 5, True)
        got, tally = p.verify_batch(ballots)
        assert got == want and tally == op.tally(ballots, want)
        got2, _ = p.verify_batch(ballots)                 # second call: tables already there
        assert got2 == want
        oq = oracle.QvParams(pk, 5, 20)
        qb = bytearray(oq.generate_batch(10, 0, 40))
        qb[3 * oq.ballot_size + oq.ballot_size - 32] ^= 1
        qb = bytes(qb)
        q = eg.QuadraticVotingParams(c, pk, 5, 20)
        gq, tq = q.verify_batch(qb)
        wq = oq.verify_batch(qb)
        assert gq == wq and tq == oq.tally(qb, wq)
        assert c.comb_table_bits() == (20, big_bits)
        if big_bits:
            assert c.selfcheck_generator_table(True, 2000, 3) == 0
        else:
            with pytest.raises(eg.EgError):
                c.selfcheck_generator_table(True, 10, 3)
    finally:
        c.close()


# ------------------------------------------------------------------ golden fixtures through the batch tier
def test_golden_encrypted_choice(eg, ctx, golden, pk):
    p = eg.ChoiceParams(ctx, pk, 5, True)
    ballot = bytes.fromhex(golden["encrypted-choice"]["packed"])
    st, tally = p.verify_batch(ballot)
    assert st == [0]
    assert tally == ballot[:320]          # a single accepted ballot: tally == its ciphertexts (canonical encodings)
    m = eg.ChoiceParams(ctx, pk, 5, False)
    mb = bytes.fromhex(golden["encrypted-multi-choice"]["packed"])
    st, tally = m.verify_batch(mb)
    assert st == [0] and tally == mb[:320]


def test_golden_qv_ballot(eg, ctx, golden, pk):
    q = eg.QuadraticVotingParams(ctx, pk, 5, 15)
    ballot = bytes.fromhex(golden["qv-ballot"]["packed"])
    assert q.ballot_size == len(ballot)
    st, tally = q.verify_batch(ballot)
    assert st == [0]
    vote_size = 64 + 32 * 5
    assert tally == b"".join(ballot[i * vote_size : i * vote_size + 64] for i in range(5))


def test_bad_public_key_is_rejected(eg, ctx):
    with pytest.raises(eg.EgError):
        eg.ChoiceParams(ctx, b"\xff" * 32, 5, True)      # invalid element (keys/mod.rs:169-170)
    with pytest.raises(eg.EgError):
        eg.ChoiceParams(ctx, b"\0" * 32, 5, True)        # identity key (keys/mod.rs:171-172)


# ------------------------------------------------------------------ batches vs the oracle, with tampering
def _tamper_choice(ballots, size, oracle, rnd):
    """Mutations mirroring choice.rs:452-475 + wire-level corruption; returns mutated bytes."""
    b = bytearray(ballots)
    n = len(b) // size
    g10 = oracle.point_mul_generator((10).to_bytes(32, "little"))
    for i in range(n):
        o = i * size
        kind = i % 10
        if kind == 1:
            b[o + 320 + 32 * rnd.randrange(1, 11)] ^= 1                   # response bit
        elif kind == 2:
            b[o + size - 32] ^= 4                                        # sum response
        elif kind == 3:
            b[o + 64 : o + 96] = b"\xff" * 32                            # invalid point
        elif kind == 4:
            b[o + 320 + 32 * 4 + 31] = 0xFF                              # non-canonical scalar
        elif kind == 5:                                                 # +10G / -10G keeps the sum proof valid
            b[o + 288 : o + 320] = oracle.point_add(bytes(b[o + 288 : o + 320]), g10)
            b[o + 224 : o + 256] = oracle.point_add(bytes(b[o + 224 : o + 256]), g10, sub=True)
        elif kind == 6:
            b[o + 32 : o + 64], b[o + 96 : o + 128] = b[o + 96 : o + 128], b[o + 32 : o + 64]   # swap two B's
        elif kind == 7:
            b[o + 320] ^= 0x10                                           # common challenge
    return bytes(b)


@pytest.mark.parametrize("n_ballots", [1, 63, 300])
def test_choice_batch_vs_oracle(eg, ctx, oracle, pk, n_ballots):
    rnd = random.Random(n_ballots)
    op = oracle.ChoiceParams(pk, 5, True)
    ballots = _tamper_choice(op.generate_batch(77, 0, n_ballots), op.ballot_size, oracle, rnd)
    want = op.verify_batch(ballots)
    p = eg.ChoiceParams(ctx, pk, 5, True)
    got, tally = p.verify_batch(ballots)
    assert got == want
    assert tally == op.tally(ballots, want)
    if n_ballots >= 63:
        kinds = {eg.status_kind(s) for s in got}
        assert {0, eg.BAD_POINT, eg.BAD_SCALAR, eg.SUM_CHALLENGE, eg.RANGE_CHALLENGE} <= kinds


def test_choice_empty_batch(eg, ctx, pk):
    p = eg.ChoiceParams(ctx, pk, 5, True)
    st, tally = p.verify_batch(b"")
    assert st == [] and tally == b"\0" * 320          # identity ciphertexts (Ciphertext::zero, encryption.rs:123-128)


def test_multi_choice_3_of_16_vs_oracle(eg, ctx, oracle, pk):
    op = oracle.ChoiceParams(pk, 16, False)
    ballots = bytearray(op.generate_batch(5, 0, 40, n_selected=3))
    ballots[3 * 2080 + 1024 + 32 * 5] ^= 1
    ballots[9 * 2080 + 100] ^= 0x80
    ballots = bytes(ballots)
    want = op.verify_batch(ballots)
    p = eg.ChoiceParams(ctx, pk, 16, False)
    got, tally = p.verify_batch(ballots)
    assert got == want and want.count(0) >= 37
    assert tally == op.tally(ballots, want)


def test_options_2_3_10_15(eg, ctx, oracle, pk):
    # sizes of tests/integration/basic.rs:164-260
    for n in (2, 3, 10, 15):
        for single in (True, False):
            op = oracle.ChoiceParams(pk, n, single)
            ballots = op.generate_batch(1000 + n, 0, 6, n_selected=max(1, n // 3))
            p = eg.ChoiceParams(ctx, pk, n, single)
            got, tally = p.verify_batch(ballots)
            assert got == [0] * 6 == op.verify_batch(ballots)
            assert tally == op.tally(ballots, got)


def test_qv_batch_vs_oracle(eg, ctx, oracle, pk):
    oq = oracle.QvParams(pk, 5, 20)
    n = 48
    ballots = bytearray(oq.generate_batch(9, 0, n))
    g = oracle.const_bytes(4)
    sz = oq.ballot_size
    vs = oq.vote_size
    # quadratic_voting.rs:433-464 style mutations
    b1 = 1 * sz
    ballots[b1 + 32 : b1 + 64] = oracle.point_add(bytes(ballots[b1 + 32 : b1 + 64]), g)                   # vote 0 ct
    b2 = 2 * sz + 5 * vs
    ballots[b2 + 32 : b2 + 64] = oracle.point_add(bytes(ballots[b2 + 32 : b2 + 64]), g, sub=True)         # credit ct
    b3 = 3 * sz + 2 * vs
    ballots[b3 + 32 : b3 + 64] = oracle.point_add(bytes(ballots[b3 + 32 : b3 + 64]), g)                   # vote 2 ct
    ballots[4 * sz + sz - 32] ^= 1                                                                       # sum response
    ballots[5 * sz + 5 * vs + 64 : 5 * sz + 5 * vs + 96] = b"\xff" * 32                                  # bad partial point
    donor = oq.generate_batch(1234, 0, 1)
    ballots[6 * sz : 6 * sz + vs] = donor[:vs]                                                           # valid proof, other value
    ballots = bytes(ballots)
    want = oq.verify_batch(ballots)
    q = eg.QuadraticVotingParams(ctx, pk, 5, 20)
    assert q.ballot_size == sz == 2144
    got, tally = q.verify_batch(ballots)
    assert got == want
    assert tally == oq.tally(ballots, want)
    assert got[1] == eg.QV_VARIANT_CHALLENGE and got[3] == (eg.QV_VARIANT_CHALLENGE | (2 << 8))
    assert got[2] == eg.QV_CREDIT_RANGE_CHALLENGE and got[4] == eg.QV_CREDIT_EQUIV_CHALLENGE
    assert eg.status_kind(got[5]) == eg.BAD_POINT


def test_tally_linearity_and_chunking(eg, ctx, oracle, pk, monkeypatch):
    # size-independent property: tally(A ++ B) == tally(A) + tally(B); small chunk forces the multi-chunk path
    monkeypatch.setenv("EG_CHUNK", "256")
    op = oracle.ChoiceParams(pk, 5, True)
    ballots = op.generate_batch(4242, 0, 700)
    p = eg.ChoiceParams(ctx, pk, 5, True)
    st, tally = p.verify_batch(ballots)
    assert st == [0] * 700
    half = 350 * op.ballot_size
    _, ta = p.verify_batch(ballots[:half])
    _, tb = p.verify_batch(ballots[half:])
    grp = eg.Ristretto(ctx)
    summed, ok = grp.element_add(ta, tb)
    assert summed == tally == op.tally(ballots, st)


# ------------------------------------------------------------------ GPU ballot generator (EncryptedChoice::new)
def _gen_on_gpu(eg, p, base_seed, first, n, n_selected=0):
    import torch

    out = torch.zeros(n * p.ballot_size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(base_seed, first, n, out.data_ptr(), n_selected=n_selected)
    p.ctx.synchronize()
    return bytes(out.cpu().numpy())


def test_generator_matches_oracle_prover(eg, ctx, oracle, pk):
    # the oracle's prover is pinned byte-for-byte by the reference's snapshots; the GPU prover must equal it
    p = eg.ChoiceParams(ctx, pk, 5, True)
    op = oracle.ChoiceParams(pk, 5, True)
    got = _gen_on_gpu(eg, p, 555, 10, 300)
    assert got == op.generate_batch(555, 10, 300)
    st, _ = p.verify_batch(got)
    assert st == [0] * 300
    m = eg.ChoiceParams(ctx, pk, 16, False)
    om = oracle.ChoiceParams(pk, 16, False)
    got = _gen_on_gpu(eg, m, 77, 0, 70, n_selected=3)
    assert got == om.generate_batch(77, 0, 70, n_selected=3)
    for n in (2, 3, 10):
        q = eg.ChoiceParams(ctx, pk, n, True)
        oq = oracle.ChoiceParams(pk, n, True)
        assert _gen_on_gpu(eg, q, 9000 + n, 0, 20) == oq.generate_batch(9000 + n, 0, 20)
    # elections beyond 32 options: a ballot's secrets live in the generator's device workspace, nothing caps the shape
    for n, single, sel in ((33, True, 0), (40, False, 7), (150, False, 4)):
        q = eg.ChoiceParams(ctx, pk, n, single)
        oq = oracle.ChoiceParams(pk, n, single)
        assert _gen_on_gpu(eg, q, 7000 + n, 3, 12, n_selected=sel) == oq.generate_batch(7000 + n, 3, 12, n_selected=sel, threads=8)
    # explicit choices with a two-word bitmask (40 options), against the oracle prover given the same flags
    q = eg.ChoiceParams(ctx, pk, 40, False)
    oq = oracle.ChoiceParams(pk, 40, False)
    mask = (1 << 39) | (1 << 32) | (1 << 31) | 1
    got = q.encrypt_selected(4321, 0, [mask, 1 << 35])
    for i, m in enumerate((mask, 1 << 35)):
        flags = [(m >> k) & 1 for k in range(40)]
        assert got[i * q.ballot_size : (i + 1) * q.ballot_size] == oq.new_ballot(flags, oracle.rng_from_u64(4321 + i))


def test_snapshot_seed_reproduced_on_gpu(eg, ctx, golden, pk, oracle):
    # Same RNG discipline as tests/snapshots.rs: the ballot drawn from seed s equals the oracle's for seed s
    p = eg.ChoiceParams(ctx, pk, 5, True)
    op = oracle.ChoiceParams(pk, 5, True)
    one = _gen_on_gpu(eg, p, 12345, 0, 1)
    rng = oracle.rng_from_u64(12345)
    flags = oracle.select_single(12345, 5)
    assert one == op.new_ballot(flags, rng)


def test_gpu_prover_reproduces_the_reference_snapshots(eg, ctx, golden, pk):
    """tests/snapshots.rs:107-131,155-161 directly on the HIP prover: seed 12345, the keypair draw skipped (rng_skip = 1), the
    snapshot's own choices / votes -> the packed bytes of `encrypted-choice`, `encrypted-multi-choice` and `qv-ballot`."""
    g = golden["encrypted-choice"]
    p = eg.ChoiceParams.single_choice(ctx, pk, g["params"]["options"])
    assert p.encrypt_selected(golden["seed"], 0, [1 << g["params"]["choice"]], rng_skip=1).hex() == g["packed"]
    g = golden["encrypted-multi-choice"]
    m = eg.ChoiceParams.multi_choice(ctx, pk, g["params"]["options"])
    mask = sum(1 << k for k, c in enumerate(g["params"]["choices"]) if c)
    assert m.encrypt_selected(golden["seed"], 0, [mask], rng_skip=1).hex() == g["packed"]
    g = golden["qv-ballot"]
    q = eg.QuadraticVotingParams(ctx, pk, g["params"]["options"], g["params"]["credits"])
    assert q.encrypt_votes(golden["seed"], 0, [g["params"]["votes"]], rng_skip=1).hex() == g["packed"]
    # the host forms refuse what EncryptedChoice::single / QuadraticVotingBallot::new would not accept
    with pytest.raises(eg.EgError):
        p.encrypt_selected(1, 0, [0b11])
    with pytest.raises(eg.EgError):
        p.encrypt_selected(1, 0, [1 << 7])
    with pytest.raises(eg.EgError):
        q.encrypt_votes(1, 0, [[3, 3, 0, 0, 0]])              # 18 credits > 15
    # explicit choices, many ballots: every one verifies and the tally counts the chosen options
    sel = [1 << (i % 5) for i in range(200)]
    st, tally = p.verify_batch(p.encrypt_selected(99, 0, sel))
    assert st == [0] * 200 and len(tally) == 320


def test_sum_of_squares_proof_on_its_own(eg, ctx, golden, pk, oracle):
    """SumOfSquaresProof::verify (mul.rs:190-260) as its own entry: the reference's `sum-sq-proof` snapshot (label b"test",
    values [1, 3, 3, 7, 5]; the snapshot holds only the proof, its ciphertexts are re-derived from the seed by the pinned oracle
    prover) is accepted by the HIP path; tampered, reordered and re-labelled variants get the oracle's verdicts."""
    k = oracle.PublicKey(pk)
    vals = golden["sum-sq-proof"]["params"]["values"]
    rng = oracle.keypair_from_seed(golden["seed"])[2]                          # the RNG after the keypair draw
    cts, proof = k.sumsq_snapshot(vals, rng)                                   # cts = sum ciphertext || value ciphertexts
    assert proof.hex() == golden["sum-sq-proof"]["packed"]
    n = len(vals)
    item = cts[64:] + cts[:64] + proof
    v = eg.SumOfSquaresVerifier(ctx, pk, n, b"test")
    assert v.item_size == len(item) == 64 * (n + 1) + 32 * (2 * n + 2)
    swapped = cts[128:192] + cts[64:128] + cts[192:] + cts[:64] + proof        # reorder two ciphertexts (mul.rs:332-361)
    bad_resp = bytearray(item); bad_resp[-1] ^= 1
    bad_pt = bytearray(item); bad_pt[0:32] = b"\xff" * 32
    batch = [item, swapped, bytes(bad_resp), bytes(bad_pt), item]
    got = v.verify_batch(b"".join(batch))
    oracle_verdict = lambda b: k.verify_sumsq(b[: 64 * n], b[64 * n : 64 * n + 64], b[64 * n + 64 :], b"test")
    assert got[0] == got[4] == 0 == oracle_verdict(item)
    assert got[1] == eg.QV_CREDIT_EQUIV_CHALLENGE == oracle_verdict(swapped)
    if int.from_bytes(bad_resp[-32:], "little") < L:                         # flipping the low bit of the top byte keeps it canonical
        assert got[2] == eg.QV_CREDIT_EQUIV_CHALLENGE == oracle_verdict(bytes(bad_resp))
    else:
        assert eg.status_kind(got[2]) == eg.BAD_SCALAR
    assert eg.status_kind(got[3]) == eg.BAD_POINT and eg.status_detail(got[3]) == 0
    other = eg.SumOfSquaresVerifier(ctx, pk, n, b"other")
    assert other.verify_batch(item) == [eg.QV_CREDIT_EQUIV_CHALLENGE] == [k.verify_sumsq(cts[64:], cts[:64], proof, b"other")]
    # 2 and 9 values, fresh proofs from the oracle prover
    for m in (2, 9):
        vv = [(3 * i + 1) % 6 for i in range(m)]
        c2, p2 = k.sumsq_snapshot(vv, oracle.rng_from_u64(700 + m))
        it = c2[64:] + c2[:64] + p2
        assert eg.SumOfSquaresVerifier(ctx, pk, m, b"test").verify_batch(it + it) == [0, 0]


def test_merlin_known_answers_on_the_gpu(eg, ctx, oracle):
    """The transcript layer (merlin 3.0.0 under src/proofs/mod.rs:39-57) checked on the device itself: the upstream merlin test
    vector and message lengths around the STROBE rate against the oracle's restatement."""
    got = ctx.merlin_challenges(b"test protocol", b"some label", [b"some data"], b"challenge", 32)
    assert got[0].hex() == "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615"
    rnd = random.Random(7)
    for n in (0, 1, 31, 32, 64, 165, 166, 167, 400):
        msgs = [bytes(rnd.getrandbits(8) for _ in range(n)) for _ in range(70)]
        for out_len in (64, 200):
            got = ctx.merlin_challenges(b"encrypted_choice_ranges", b"enc", msgs, b"c", out_len)
            for m, g in zip(msgs, got):
                t = oracle.Merlin(b"encrypted_choice_ranges"); t.append(b"enc", m)
                assert g == t.challenge(b"c", out_len), (n, out_len)


def test_merlin_entry_at_its_own_edges(eg, ctx, oracle):
    """eg_merlin_challenge_batch where its own arguments meet the 166-byte STROBE block: protocol, message and challenge labels of 0, 1,
    165, 166, 167 and 255 bytes in every combination (bytes 1..255, one >= 0x80 at least), message lengths 0, 163..167 and 331..333
    with every challenge length of 1, 165, 166, 167, 332 and 1024 bytes, batches of 1, 63, 64, 65 and 257 distinct messages - all
    against the oracle's transcript - and what the entry refuses."""
    import ctypes as C

    import transcript_scripts as ts

    labels, msg_lens, out_lens, ns = (0, 1, 165, 166, 167, 255), (0, 163, 164, 165, 166, 167, 331, 332, 333), (1, 165, 166, 167, 332, 1024), \
        (1, 63, 64, 65, 257)
    cases = [(p, m, c, msg_lens[(k // 6) % 9], out_lens[k % 6]) for k, (p, m, c) in
             enumerate((p, m, c) for p in labels for m in labels for c in labels)]
    cases += [(labels[k % 6], labels[(k // 6) % 6], labels[(k // 2) % 6], ml, ol) for k, (ml, ol) in
              enumerate((ml, ol) for ml in msg_lens for ol in out_lens)]
    assert {(p, m, c) for p, m, c, _, _ in cases} >= {(p, m, c) for p in labels for m in labels for c in labels}
    assert {(ml, ol) for _, _, _, ml, ol in cases} == {(ml, ol) for ml in msg_lens for ol in out_lens}
    rnd = random.Random(71)
    for k, (p, m, c, ml, ol) in enumerate(cases):
        n = ns[k % 5]
        proto, msg_label, chal_label = ts.label_bytes(p, 50), ts.label_bytes(m, 51), ts.label_bytes(c, 52)
        msgs = [i.to_bytes(2, "little") + rnd.getrandbits(8 * ml).to_bytes(ml, "little")[2:] if ml else b"" for i in range(n)]
        got = ctx.merlin_challenges(proto, msg_label, msgs, chal_label, ol)
        assert len(got) == n
        for i, (msg, g) in enumerate(zip(msgs, got)):
            t = oracle.Merlin(proto); t.append(msg_label, msg)
            assert g == t.challenge(chal_label, ol), (p, m, c, ml, ol, n, i)
    long_label = ts.label_bytes(256, 53)
    for args in ((long_label, b"m", b"c", 64), (b"p", long_label, b"c", 64), (b"p", b"m", long_label, 64), (b"p", b"m", b"c", 0),
                 (b"p", b"m", b"c", 1025)):
        with pytest.raises(eg.EgError):
            ctx.merlin_challenges(args[0], args[1], [b"msg"], args[2], args[3])
    lib, out = eg._load(), C.create_string_buffer(1025)
    BAD_ARG = -3                                      # include/eg_hip.h: EG_ERR_BAD_ARG
    assert lib.eg_merlin_challenge_batch(ctx._h, 1, long_label, 256, b"m", 1, b"msg", 3, b"c", 1, out, 64) == BAD_ARG
    assert lib.eg_merlin_challenge_batch(ctx._h, 1, b"p", 1, long_label, 256, b"msg", 3, b"c", 1, out, 64) == BAD_ARG
    assert lib.eg_merlin_challenge_batch(ctx._h, 1, b"p", 1, b"m", 1, b"msg", 3, long_label, 256, out, 64) == BAD_ARG
    assert lib.eg_merlin_challenge_batch(ctx._h, 1, b"p", 1, b"m", 1, b"msg", 3, b"c", 1, out, 0) == BAD_ARG
    assert lib.eg_merlin_challenge_batch(ctx._h, 1, b"p", 1, b"m", 1, b"msg", 3, b"c", 1, out, 1025) == BAD_ARG
    assert lib.eg_merlin_challenge_batch(ctx._h, 1, b"p", 1, b"m", 1, b"msg", 3, b"c", 1, out, 1024) == 0


# ------------------------------------------------------------------ PublicKey::verify_zero / verify_bool / verify_range
def test_golden_single_ciphertext_proofs(eg, ctx, golden, pk, oracle):
    z = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.ZERO)
    b = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.BOOL)
    r = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.RANGE, 100)
    zero = bytes.fromhex(golden["zero-encryption"]["packed"])
    boo = bytes.fromhex(golden["bool-encryption"]["packed"])
    rng = bytes.fromhex(golden["range-encryption"]["packed"])
    assert (z.item_size, b.item_size, r.item_size) == (128, 160, len(rng))
    assert z.verify_batch(zero) == [0] and b.verify_batch(boo) == [0] and r.verify_batch(rng) == [0]
    # tampering and batches against the oracle
    k = oracle.PublicKey(pk)
    rs = oracle.rng_from_u64(99)
    pr = oracle.PreparedRange(100)
    zs, bs, rgs = [], [], []
    for i in range(40):
        zs.append(bytearray(k.encrypt_zero(rs)))
        bs.append(bytearray(k.encrypt_bool(bool(i & 1), rs)))
        rgs.append(bytearray(k.encrypt_range(pr, (i * 7) % 100, rs)))
        if i % 5 == 1:
            zs[-1][100] ^= 1; bs[-1][70] ^= 2; rgs[-1][len(rng) - 5] ^= 1
        if i % 5 == 2:
            zs[-1][0:32] = b"\xff" * 32; bs[-1][96 + 31] = 0xFF; rgs[-1][64:96] = b"\xff" * 32
    zb, bb, rb = b"".join(map(bytes, zs)), b"".join(map(bytes, bs)), b"".join(map(bytes, rgs))
    assert z.verify_batch(zb) == [k.verify_zero(bytes(x)) for x in zs]
    assert b.verify_batch(bb) == [k.verify_bool(bytes(x)) for x in bs]
    want = [k.verify_range(pr, bytes(x)) for x in rgs]
    assert r.verify_batch(rb) == want and 0 in want and eg.RANGE_CHALLENGE in want


@pytest.mark.parametrize("upper_bound", [2, 12, 15, 20, 50, 1000, 65536, 1000000])
def test_range_proofs_various_bounds(eg, ctx, oracle, pk, upper_bound):
    # bounds of range.rs:708 (range_proof_basics) plus the extremes
    k = oracle.PublicKey(pk)
    pr = oracle.PreparedRange(upper_bound)
    rs = oracle.rng_from_u64(upper_bound)
    items = b"".join(k.encrypt_range(pr, v % upper_bound, rs) for v in (0, 1, 10, upper_bound - 1))
    r = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.RANGE, upper_bound)
    assert r.item_size == 64 + pr.proof_size
    assert r.verify_batch(items) == [0, 0, 0, 0]


# ------------------------------------------------------------------ C++ host mirror + the voting example
def test_cpp_voting_example(tmp_path):
    """examples/voting.cpp = examples/voting.rs:179-269 (`vote` and `quadratic_vote`) on the GPU backend through
    include/elastic_elgamal_hip.hpp"""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", f"-I{root / 'include'}", str(root / "examples" / "voting.cpp"),
                           f"-L{root / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{root / 'elastic_elgamal_amd'}",
                           "-o", str(exe)])
    out = subprocess.run([str(exe), "200", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "199 of 200 ballots verified" in out.stdout and "voter #4 rejected" in out.stdout
    assert "OK: the decrypted totals equal the expected ones" in out.stdout
    # Args::quadratic_vote (examples/voting.rs:219-269): the voters' own votes, expected totals, max_votes-sized lookup table
    out = subprocess.run([str(exe), "--qv", "150", "4", "20", "11"], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "149 of 150 quadratic-voting ballots verified" in out.stdout and "voter #4 rejected" in out.stdout
    assert "OK: the decrypted totals equal the expected ones" in out.stdout
    # the ballots as serde_json text, one ballot at a time, through the C++ mirror of the streaming entry (examples/voting.rs:195-198)
    out = subprocess.run([str(exe), "--json", "700", "5", "9"], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "(700 ballots went through the JSON stream one at a time)" in out.stdout
    assert "699 of 700 ballots verified" in out.stdout and "voter #4 rejected" in out.stdout
    assert "OK: the decrypted totals equal the expected ones" in out.stdout
    # ... and with ONE parser for two devices, every ballot's text handed over without a copy (JsonStream over several params objects,
    # feed_owned: eg_verify_choice_json_begin_multi / eg_verify_json_feed_owned through the C++ mirror)
    out = subprocess.run([str(exe), "--json", "--devices", "2", "900", "5", "13"], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "(900 ballots went through the JSON stream one at a time, one parser for all devices, blocks handed over)" in out.stdout
    assert "899 of 900 ballots verified" in out.stdout and "OK: the decrypted totals equal the expected ones" in out.stdout
    # the same elections through the in-process multi-GPU entry (two contexts; both on GPU 0 when the box has one GPU)
    for args in (["--devices", "2", "300", "5", "3"], ["--qv", "--devices", "2", "120", "3", "10", "5"]):
        out = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=240)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "OK: the decrypted totals equal the expected ones" in out.stdout


def test_cpp_shim_calls(tmp_path):
    """tests/cpp/shim_calls.cpp: every primitive-tier entry point with n = 1, the way the `Group` shim of INTEGRATION.md section 3 calls
    them (Element * &Scalar, From<u64>, add / sub / neg, vartime_* ...), checked against each other through group identities
    (group/mod.rs:183-255); prints the cost of one call (kept in profiles/r04_shim_call_latency.txt)."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "shim_calls"
    subprocess.check_call(["g++", "-std=c++17", "-O2", f"-I{root / 'include'}", str(root / "tests" / "cpp" / "shim_calls.cpp"),
                           f"-L{root / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{root / 'elastic_elgamal_amd'}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK: every identity holds" in out.stdout and "vartime_double_mul_generator" in out.stdout
    print(out.stdout)


def test_cpp_tally_exchange_example(tmp_path):
    """examples/tally_exchange.cpp: the one collective of the path through librccl directly (eg_*_tally_encode_device -> ncclAllGather
    -> eg_points_sum_device on one stream), the recipe for a host that is not Python; one rank on the box's one GPU."""
    import os
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "tally_exchange"
    subprocess.check_call(["hipcc", "-std=c++17", f"-I{root / 'include'}", str(root / "examples" / "tally_exchange.cpp"),
                           f"-L{root / 'elastic_elgamal_amd'}", "-leg_hip", "-lrccl", f"-Wl,-rpath,{root / 'elastic_elgamal_amd'}",
                           "-o", str(exe)])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([str(exe), "50000", "5", "9"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK: the exchanged tally equals the engine's own tally, 50000 of 50000 ballots accepted" in out.stdout
    assert "undecodable encodings 0" in out.stdout


def test_qv_generator_matches_oracle_prover(eg, ctx, oracle, pk):
    import torch

    for options, credits, n in ((5, 20, 96), (5, 15, 24), (5, 100, 8), (12, 200, 6), (20, 1000, 4), (3, 10000, 4), (1, 1, 5)):
        q = eg.QuadraticVotingParams(ctx, pk, options, credits)
        oq = oracle.QvParams(pk, options, credits)
        out = torch.zeros(n * q.ballot_size, dtype=torch.uint8, device="cuda")
        q.encrypt_batch_device(31, 5, n, out.data_ptr())
        ctx.synchronize()
        got = bytes(out.cpu().numpy())
        assert got == oq.generate_batch(31, 5, n, threads=8), (options, credits)
        st, _ = q.verify_batch(got)
        assert st == [0] * n


# ------------------------------------------------------------------ BASELINE.json full sizes, size-independent properties
@pytest.mark.parametrize("workload,n", [("single", 1_000_000), ("multi", 1_000_000), ("qv", 1_000_000), ("single", 10_000_000)])
def test_full_size_properties(eg, ctx, oracle, pk, workload, n):
    """BASELINE.json configs[1] (1M single-choice), configs[3] (1M multi-choice 3-of-16), configs[2] (1M quadratic voting,
    5 options / 20 credits) and the whole 10M-ballot batch of configs[4] on one GPU (chunked by the engine), all at full
    size: ballots generated on the GPU, 1 % tampered.  Properties: exactly the tampered ballots are rejected;
    tally(A ++ B) == tally(A) + tally(B); verdicts and tally of a random sample are bit-exact against the oracle."""
    import torch

    if workload == "single":
        p = eg.ChoiceParams(ctx, pk, 5, True); op = oracle.ChoiceParams(pk, 5, True); kw = {}
    elif workload == "multi":
        p = eg.ChoiceParams(ctx, pk, 16, False); op = oracle.ChoiceParams(pk, 16, False); kw = {"n_selected": 3}
    else:
        p = eg.QuadraticVotingParams(ctx, pk, 5, 20); op = oracle.QvParams(pk, 5, 20); kw = {}
    sz = p.ballot_size
    d = torch.empty(n * sz, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(2026, 0, n, d.data_ptr(), **kw)
    ctx.synchronize()
    g = torch.Generator(device="cpu").manual_seed(n)
    bad = torch.randperm(n, generator=g)[: n // 100].cuda()
    # flip one bit of the LAST response scalar of the ballot (keeps it canonical with overwhelming probability)
    view = d.view(n, sz)
    view[bad, sz - 32] ^= 1
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    p.tally_reset()
    p.verify_batch_device(n, d.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize()
    whole = p.tally_encode()
    rejected = torch.nonzero(st != 0).flatten()
    assert torch.equal(torch.sort(rejected).values, torch.sort(bad).values)
    # linearity over a split of the batch
    half = (n // 2)
    p.tally_reset()
    p.verify_batch_device(half, d.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize()
    ta = p.tally_encode()
    p.tally_reset()
    p.verify_batch_device(n - half, d.data_ptr() + half * sz, st.data_ptr() + 4 * half, stream)
    torch.cuda.synchronize()
    tb = p.tally_encode()
    summed, ok = eg.Ristretto(ctx).element_add(ta, tb)
    assert summed == whole and set(ok) == {1}
    # The oracle at full size (VERDICT r5 task 3): EVERY tampered ballot (n / 100) plus 20 000 drawn at random, through the host form in
    # one call - verdicts word for word and the tally of the sample.  16 threads: ~12.7 k/s single, 4.8 k/s multi, 3.8 k/s QV.  The 10 M
    # batch keeps a 64-ballot sample plus all tampered ballots of one 1.25 M slab (the slab of one rank of configs[4]).
    st.zero_()
    p.tally_reset()
    p.verify_batch_device(n, d.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize()
    if n <= 1_000_000:
        idx = torch.cat([bad, torch.randperm(n, generator=g)[:20_000].cuda()])
    else:
        slab = bad[(bad >= 1_250_000 * 3) & (bad < 1_250_000 * 4)]
        idx = torch.cat([slab, torch.randperm(n, generator=g)[:64].cuda()])
        assert 11_000 < len(slab) < 14_000
    sample = bytes(view[idx].cpu().numpy())
    want = op.verify_batch(sample, threads=16)
    assert [int(v) & 0xFFFFFFFF for v in st[idx].cpu().tolist()] == want          # the verdicts of the FULL-SIZE run, word for word
    assert want.count(0) >= (20_000 if n <= 1_000_000 else 64) * 0.98 and want[: len(idx) - (20_000 if n <= 1_000_000 else 64)].count(0) == 0
    got, gt = p.verify_batch(sample)
    assert got == want and gt == op.tally(sample, want)


# ------------------------------------------------------------------ degenerate inputs
def test_degenerate_points_and_scalars(eg, ctx, oracle, pk):
    """Identity elements (all-zero encodings are valid ristretto points), zero and l-1 scalars, repeated points:
    whatever the reference's arithmetic yields, the GPU must report the same verdict bits as the oracle."""
    rnd = random.Random(99)
    op = oracle.ChoiceParams(pk, 5, True)
    p = eg.ChoiceParams(ctx, pk, 5, True)
    base = bytearray(op.generate_batch(606, 0, 24))
    sz = op.ballot_size
    zero32, lm1 = b"\0" * 32, (L - 1).to_bytes(32, "little")
    g = oracle.const_bytes(4)
    def put(i, item, val):
        base[i * sz + 32 * item : i * sz + 32 * item + 32] = val
    put(0, 0, zero32)                      # R_0 = identity
    put(1, 1, zero32)                      # B_0 = identity
    for it in range(10): put(2, it, zero32)   # every ciphertext element = identity
    put(3, 10, zero32)                     # common challenge = 0
    put(4, 11, zero32); put(4, 12, zero32)  # responses = 0
    put(5, 10, lm1)                        # challenge = l - 1
    put(6, 13, lm1)
    put(7, 21, zero32); put(7, 22, zero32)  # sum proof (0, 0)
    for it in range(10): put(8, it, g)      # all elements = generator
    put(9, 0, bytes(base[9 * sz + 32 : 9 * sz + 64]))   # R_0 = B_0
    put(10, 2, pk); put(10, 3, pk)          # ciphertext made of the public key
    for it in range(23): put(11, it, zero32)  # entirely zero ballot
    ballots = bytes(base)
    want = op.verify_batch(ballots)
    got, tally = p.verify_batch(ballots)
    assert got == want
    assert tally == op.tally(ballots, want)
    assert want[:12].count(0) == 0 and want[12:] == [0] * 12
    # the same through the primitive tier: identity / zero-scalar corner cases of the scalar multiplication
    grp = eg.Ristretto(ctx)
    ks = [zero32, (1).to_bytes(32, "little"), lm1, (8).to_bytes(32, "little")]
    pts = [zero32, g, pk, zero32]
    out, ok = grp.vartime_double_mul_generator(b"".join(ks), b"".join(pts), b"".join(reversed(ks)))
    for i in range(4):
        assert out[32 * i : 32 * i + 32] == oracle.point_double_mul_generator(ks[i], pts[i], ks[3 - i])


def test_reference_rejection_vectors_on_the_hip_path(eg, ctx, grp, oracle, pk, rejections):
    """The REJECTING inputs of the reference's own unit tests (tests/golden/rejections_ristretto.json <- src/serde.rs:403, :428, :484,
    :511) on the HIP path: eg_point_roundtrip_batch refuses the non-element (and the all-ones-top-byte string as an element),
    eg_scalar_is_canonical_batch refuses the non-canonical scalar; a ballot that carries either in ANY of its 32-byte slots gets
    BAD_POINT / BAD_SCALAR with that slot's index (oracle agrees; serde.rs:197-198, 260-261 refuse it at deserialisation), and the JSON
    entry gives the same verdicts when the ballots carry the reference's base64url strings themselves."""
    import json
    from elastic_elgamal_amd import serde

    bad_pt, bad_sc = bytes.fromhex(rejections["non_element"]["hex"]), bytes.fromhex(rejections["non_canonical_scalar"]["hex"])
    good_pt = oracle.const_bytes(4)
    out, ok = grp.element_roundtrip(bad_pt + good_pt + bytes.fromhex(rejections["element_helper_invalid_element"]["hex"]) + bytes(32))
    assert list(ok) == [0, 1, 0, 1] and out[32:64] == good_pt and out[96:] == bytes(32)
    assert list(grp.deserialize_scalar_ok(bad_sc + sc(5) + bad_pt + (L - 1).to_bytes(32, "little") + L.to_bytes(32, "little"))) \
        == [0, 1, 1 if int.from_bytes(bad_pt, "little") < L else 0, 1, 0]
    _, ok = grp.vartime_double_mul_generator(sc(3) * 2, bad_pt + good_pt, sc(4) * 2)      # a product over the non-element is refused as well
    assert list(ok) == [0, 1]
    # single-choice ballots, 5 options: 23 items (10 elements, 13 scalars); ballot i carries the bad value in item i
    op = oracle.ChoiceParams(pk, 5, True)
    p = eg.ChoiceParams(ctx, pk, 5, True)
    sz = op.ballot_size
    raw = bytearray(op.generate_batch(31, 0, 40))
    for item in range(23):
        raw[item * sz + 32 * item : item * sz + 32 * item + 32] = bad_pt if item < 10 else bad_sc
    raw[23 * sz + 32 * 9 : 23 * sz + 32 * 10] = bad_pt              # two bad items: the FIRST one is reported
    raw[23 * sz + 32 * 4 : 23 * sz + 32 * 5] = bad_pt
    raw[24 * sz + 32 * 22 : 24 * sz + 32 * 23] = bad_sc            # a bad element beats a bad scalar that comes later in the ballot ...
    raw[24 * sz + 32 * 7 : 24 * sz + 32 * 8] = bad_pt
    raw = bytes(raw)
    want = op.verify_batch(raw)
    assert want[:23] == [(eg.BAD_POINT if item < 10 else eg.BAD_SCALAR) | (item << 8) for item in range(23)]
    assert want[23] == eg.BAD_POINT | (4 << 8) and want[24] == eg.BAD_POINT | (7 << 8) and want[25:] == [0] * 15
    got, tally = p.verify_batch(raw)
    assert got == want and tally == op.tally(raw, want)
    # quadratic voting: a vote ciphertext, a partial ciphertext of the credit proof, a ring response, the sum-of-squares responses
    oq = oracle.QvParams(pk, 5, 20)
    q = eg.QuadraticVotingParams(ctx, pk, 5, 20)
    qsz = oq.ballot_size
    n_items = qsz // 32
    qraw = bytearray(oq.generate_batch(32, 0, n_items + 3, threads=8))
    is_point = []
    for v in range(5):
        is_point += [True, True] + [False] * 6            # ciphertext, common challenge + 5 responses (ring of 5, no partials)
    is_point += [True, True, True, True] + [False] * 11    # credit: ciphertext, one partial ciphertext, challenge + 7 + 3 responses
    is_point += [False] * 12                               # sum of squares: challenge, 10 responses, sum response
    assert len(is_point) == n_items
    for item in range(n_items):
        qraw[item * qsz + 32 * item : item * qsz + 32 * item + 32] = bad_pt if is_point[item] else bad_sc
    qraw = bytes(qraw)
    qwant = oq.verify_batch(qraw)
    assert qwant[:n_items] == [(eg.BAD_POINT if is_point[i] else eg.BAD_SCALAR) | (i << 8) for i in range(n_items)] and qwant[n_items:] == [0] * 3
    qgot, qtally = q.verify_batch(qraw)
    assert qgot == qwant and qtally == oq.tally(qraw, qwant)
    # the same ballots as JSON text with the reference's strings in place (base64url, unpadded: serde.rs:19-80)
    objs = [serde.unpack_encrypted_choice(raw[i * sz : (i + 1) * sz], 5, True) for i in range(40)]
    text = json.dumps(objs)
    assert text.count(rejections["non_element"]["b64"]) == 10 + 3 and text.count(rejections["non_canonical_scalar"]["b64"]) == 13 + 1
    p.tally_reset()
    jgot, jtally = p.verify_json(text)
    assert jgot == want and jtally == tally


# ------------------------------------------------------------------ tally stage: decryption shares
def test_threshold_tally_end_to_end(eg, ctx, oracle):
    """examples/voting.rs:122-177 shape with a 7-of-10 key: verify ballots, tally, every tallier's decryption share is
    verified on the GPU (PublicKeySet::verify_share), 7 shares are combined (Lagrange in the exponent) and the totals
    are read off a discrete-log table; a forged share is rejected."""
    from elastic_elgamal_amd import tally as T

    rnd = random.Random(2024)
    shares_n, threshold, n_opt, votes = 10, 7, 5, 60
    coeffs = [rnd.randrange(L) for _ in range(threshold)]               # Shamir polynomial, secret = coeffs[0]
    f = lambda x: sum(c * pow(x, k, L) for k, c in enumerate(coeffs)) % L
    sk_shares = [f(i + 1) for i in range(shares_n)]
    shared_key = oracle.point_mul_generator(sc(coeffs[0]))
    part_keys = [oracle.point_mul_generator(sc(s)) for s in sk_shares]
    grp = eg.Ristretto(ctx)
    params = eg.ChoiceParams(ctx, shared_key, n_opt, True)
    ballots = params.encrypt_batch(55, 0, votes)
    expected = [0] * n_opt
    for i in range(votes):
        expected[oracle.select_single(55 + i, n_opt).index(1)] += 1
    st, totals = params.verify_batch(ballots)
    assert st == [0] * votes
    rng = oracle.rng_from_u64(1)
    table = T.DiscreteLogTable(grp, range(votes + 1))
    verifiers = [eg.DecryptionShareVerifier(ctx, shared_key, shares_n, threshold, i, part_keys[i]) for i in range(shares_n)]
    got = []
    for k in range(n_opt):
        ct = totals[64 * k : 64 * k + 64]
        verified = []
        for i in rnd.sample(range(shares_n), shares_n):
            share = oracle.decryption_share_new(sc(sk_shares[i]), ct[:32], shares_n, threshold, shared_key, i, rng)
            item = ct[:32] + share
            assert verifiers[i].verify_batch(item) == [oracle.decryption_share_verify(part_keys[i], shares_n, threshold, shared_key, i, item)] == [0]
            bad = bytearray(item); bad[70] ^= 1
            assert verifiers[i].verify_batch(bytes(bad)) == [eg.SUM_CHALLENGE]
            assert verifiers[(i + 1) % shares_n].verify_batch(item) == [eg.SUM_CHALLENGE]     # other participant's key
            verified.append((i, share[:32]))
        assert T.combine_shares(grp, threshold, verified[: threshold - 1], n_shares=shares_n) is None
        dh = T.combine_shares(grp, threshold, verified, n_shares=shares_n)
        assert dh == T.combine_shares(grp, threshold, list(reversed(verified[:threshold])), n_shares=shares_n)   # any order of the same shares
        assert dh == oracle.point_multi_mul(sc(coeffs[0]), ct[:32])                       # [x]R for the shared secret x
        got.append(T.decrypt_total(grp, table, ct, dh))
    assert got == expected and sum(got) == votes
    # Params::combine_shares panics on an index beyond the key set; duplicates cannot be interpolated: both are refused
    with pytest.raises(eg.EgError):
        T.combine_shares(grp, threshold, [(shares_n, verified[0][1])] + verified[1:], n_shares=shares_n)
    with pytest.raises(eg.EgError):
        T.combine_shares(grp, threshold, [verified[0]] * threshold, n_shares=shares_n)
    # DiscreteLogTable: zero is always found (identity), values outside the table are not
    assert table.get(b"\0" * 32) == 0
    assert table.get(oracle.point_mul_generator(sc(votes))) == votes
    assert table.get(oracle.point_mul_generator(sc(votes + 1))) is None
    # the wide comb tables on request (eg_*_prepare_wide_tables): same verdicts afterwards
    params.prepare_wide_tables()
    assert ctx.comb_table_bits()[1] != 0
    assert params.verify_batch(ballots)[0] == [0] * votes


# ------------------------------------------------------------------ unusual election shapes
@pytest.mark.parametrize("n,single", [(1, True), (1, False), (2, True), (7, True), (32, False), (33, True), (40, False)])
def test_choice_unusual_option_counts(eg, ctx, oracle, pk, n, single):
    # 1 option (one ring), 32/33/40 options (more than 32 commitments per stage: several batched inversions)
    op = oracle.ChoiceParams(pk, n, single)
    ballots = bytearray(op.generate_batch(n * 31, 0, 5, n_selected=min(n, 2)))
    ballots[1 * op.ballot_size + 64 * n + 32] ^= 1          # first response of ballot 1
    ballots[3 * op.ballot_size + 5] ^= 0x40                 # an element of ballot 3
    ballots = bytes(ballots)
    want = op.verify_batch(ballots)
    p = eg.ChoiceParams(ctx, pk, n, single)
    got, tally = p.verify_batch(ballots)
    assert got == want and want[0] == 0 and want[1] != 0
    assert tally == op.tally(ballots, want)


@pytest.mark.parametrize("options,credits", [(1, 1), (2, 4), (3, 9), (5, 25), (4, 100), (8, 36)])
def test_qv_unusual_parameters(eg, ctx, oracle, pk, options, credits):
    # quadratic_voting.rs:420-431 uses (5, 25); others exercise 1-ring and 3-ring decompositions and long rings
    oq = oracle.QvParams(pk, options, credits)
    q = eg.QuadraticVotingParams(ctx, pk, options, credits)
    assert q.ballot_size == oq.ballot_size
    ballots = bytearray(oq.generate_batch(credits, 0, 6))
    ballots[2 * oq.ballot_size + oq.ballot_size - 1] ^= 1 if ballots[2 * oq.ballot_size + oq.ballot_size - 1] & 0x0F else 2
    ballots[4 * oq.ballot_size + 40] ^= 8
    ballots = bytes(ballots)
    want = oq.verify_batch(ballots)
    got, tally = q.verify_batch(ballots)
    assert got == want and want.count(0) >= 4
    assert tally == oq.tally(ballots, want)


def test_concurrent_host_calls_are_serialised(eg, ctx, oracle, pk):
    """eg_hip.h: entry points may be called from any thread; one context serialises them."""
    import threading
    op = oracle.ChoiceParams(pk, 4, True)
    p = eg.ChoiceParams.single_choice(ctx, pk, 4)
    q = eg.QuadraticVotingParams(ctx, pk, 3, 9)
    oq = oracle.QvParams(pk, 3, 9)
    ballots = op.generate_batch(77, 0, 40)
    qballots = oq.generate_batch(78, 0, 12)
    want, wantq = op.verify_batch(ballots), oq.verify_batch(qballots)
    grp = eg.Ristretto(ctx)
    ks = b"".join(sc(i + 1) for i in range(64))
    want_pts = b"".join(oracle.point_mul_generator(sc(i + 1)) for i in range(64))
    errors = []

    def worker(kind):
        try:
            for _ in range(6):
                if kind == 0:
                    assert p.verify_batch(ballots)[0] == want
                elif kind == 1:
                    assert q.verify_batch(qballots)[0] == wantq
                else:
                    assert grp.mul_generator(ks) == want_pts
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(k % 3,)) for k in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    # a one-shot JSON call does not hold the context's lock for its length (its worker thread takes it piece by piece), yet it is ONE call on
    # the params object for other threads: their verify / tally / JSON calls on the same object wait for it instead of being refused
    import json
    from elastic_elgamal_amd import serde
    sz = op.ballot_size
    text = json.dumps([serde.unpack_encrypted_choice(ballots[i * sz : (i + 1) * sz], 4, True) for i in range(40)] * 50)

    def worker2(kind):
        try:
            for _ in range(5):
                if kind == 0:
                    assert p.verify_json(text)[0] == want * 50
                elif kind == 1:
                    assert p.verify_batch(ballots)[0] == want
                elif kind == 2:
                    assert len(p.tally_encode()) == 64 * 4
                else:
                    st = p.json_stream(threads=2)
                    st.feed(text)
                    assert st.end()[0] == want * 50
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker2, args=(k,)) for k in (0, 1, 2, 0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_large_election_chunks_follow_device_memory(eg, ctx, oracle, pk):
    """150 options: ~1.6 MB of comb tables per ballot, so the engine must shrink its chunks below EG_CHUNK to fit the
    device.  ~98k INDEPENDENT ballots made by the GPU prover (4 of 150 options each); verdicts of a sample and of the
    tampered ballots are the oracle's, and the tally is linear over a split of the batch."""
    import torch

    n_opt, n = 150, 98304
    p = eg.ChoiceParams(ctx, pk, n_opt, False)
    op = oracle.ChoiceParams(pk, n_opt, False)
    sz = p.ballot_size
    d = torch.empty(n * sz, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(909, 0, n, d.data_ptr(), n_selected=4)
    ctx.synchronize()
    view = d.view(n, sz)
    head = bytes(view[:24].cpu().numpy())
    assert head == op.generate_batch(909, 0, 24, n_selected=4, threads=8)          # the prover itself, on this shape
    bad = torch.tensor([0, 7, n // 2, n - 1], device="cuda")
    view[bad, sz - 32] ^= 1
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    p.tally_reset()
    p.verify_batch_device(n, d.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize()
    assert torch.nonzero(st != 0).flatten().tolist() == sorted(bad.tolist())
    whole = p.tally_encode()
    half = n // 2
    p.tally_reset()
    p.verify_batch_device(half, d.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize()
    ta = p.tally_encode()
    p.tally_reset()
    p.verify_batch_device(n - half, d.data_ptr() + half * sz, st.data_ptr() + 4 * half, stream)
    torch.cuda.synchronize()
    tb = p.tally_encode()
    grp = eg.Ristretto(ctx)
    assert grp.element_add(ta, tb)[0] == whole
    idx = [0, 7, 8, 100, n // 2, n // 2 + 1, n - 2, n - 1]
    sample = b"".join(bytes(view[i].cpu().numpy()) for i in idx)
    got, gt = p.verify_batch(sample)
    want = op.verify_batch(sample, threads=8)
    assert got == want and gt == op.tally(sample, want) and want.count(0) == 4


def test_maximum_election_sizes(eg, ctx, oracle, pk):
    """The largest elections the C ABI accepts (eg_hip.h: 4000 options for choice ballots, 256 options / 100 000 credits for
    quadratic voting).  Up to the oracle's capacity (256 options) prover and verifier are compared with it; beyond it the checks
    are properties: GPU-made ballots verify, a flipped bit is caught, the tally is the sum of the accepted ciphertexts."""
    grp = eg.Ristretto(ctx)
    # multi-choice, 256 options: GPU prover == oracle prover, verdicts == oracle
    m = eg.ChoiceParams.multi_choice(ctx, pk, 256)
    om = oracle.ChoiceParams(pk, 256, False)
    b = bytearray(_gen_on_gpu(eg, m, 3, 0, 4, n_selected=7))
    assert bytes(b) == om.generate_batch(3, 0, 4, n_selected=7, threads=8)
    b[2 * m.ballot_size + 64 * 256 + 32 * 100] ^= 1
    st, tally = m.verify_batch(bytes(b))
    assert st == om.verify_batch(bytes(b), threads=8) and st.count(0) == 3 and tally == om.tally(bytes(b), st)
    # quadratic voting, 256 options / 100 000 credits (7-ring credit range, 4-ring vote range, 255 712-byte ballots)
    q = eg.QuadraticVotingParams(ctx, pk, 256, 100000)
    oq = oracle.QvParams(pk, 256, 100000)
    assert q.ballot_size == oq.ballot_size == 255712
    import torch
    out = torch.zeros(2 * q.ballot_size, dtype=torch.uint8, device="cuda")
    q.encrypt_batch_device(3, 0, 2, out.data_ptr())
    ctx.synchronize()
    qb = bytearray(out.cpu().numpy().tobytes())
    assert bytes(qb) == oq.generate_batch(3, 0, 2, threads=8)
    qb[q.ballot_size + q.ballot_size - 1] ^= 1 if qb[q.ballot_size + q.ballot_size - 1] & 0x0F else 2
    st, tally = q.verify_batch(bytes(qb))
    assert st == oq.verify_batch(bytes(qb), threads=8) and st[0] == 0 and st[1] != 0 and tally == oq.tally(bytes(qb), st)
    # single-choice, 4000 options (beyond the oracle): properties only
    p = eg.ChoiceParams.single_choice(ctx, pk, 4000)
    assert p.ballot_size == 4000 * 64 + 32 * 8001 + 64
    pb = bytearray(p.encrypt_selected(11, 0, [1 << 3999, 1 << 0, 1 << 1234]))
    st, tally = p.verify_batch(bytes(pb))
    assert st == [0, 0, 0]
    summed = grp.element_add(grp.element_add(bytes(pb[: 256000]), bytes(pb[p.ballot_size : p.ballot_size + 256000]))[0],
                             bytes(pb[2 * p.ballot_size : 2 * p.ballot_size + 256000]))[0]
    assert tally == summed
    pb[p.ballot_size + 256000 + 32 * 4001] ^= 1                        # a ring response of ballot 1
    pb[2 * p.ballot_size + p.ballot_size - 32] ^= 1                    # the sum-proof response of ballot 2
    st, _ = p.verify_batch(bytes(pb))
    assert st == [0, eg.RANGE_CHALLENGE, eg.SUM_CHALLENGE]


@pytest.mark.parametrize("options,credits", [(12, 200), (20, 1000), (3, 10000)])
def test_qv_large_parameters_oracle_ballots(eg, ctx, oracle, pk, options, credits):
    """Large quadratic-voting shapes (multi-ring vote ranges, long rings): ballots from the oracle prover, tampered in every
    section."""
    oq = oracle.QvParams(pk, options, credits)
    q = eg.QuadraticVotingParams(ctx, pk, options, credits)
    n = 24
    ballots = bytearray(oq.generate_batch(17, 0, n, threads=8))
    sz = q.ballot_size
    assert sz * n == len(ballots)
    rnd = random.Random(options * 1000 + credits)
    for b in range(0, n, 2):                       # every other ballot: flip one bit somewhere in the ballot
        ballots[b * sz + rnd.randrange(sz)] ^= 1 << rnd.randrange(8)
    want = oq.verify_batch(bytes(ballots), threads=8)
    assert any(w != 0 for w in want) and any(w == 0 for w in want)
    got, tally = q.verify_batch(bytes(ballots))
    assert got == want
    assert tally == oq.tally(bytes(ballots), want)


@pytest.mark.parametrize("workload", ["single", "multi", "qv"])
def test_random_bit_flips_match_oracle(eg, ctx, oracle, pk, workload):
    """Differential fuzz: 1-3 random bit flips anywhere in each ballot (points, scalars, challenges); the status words
    (kind and detail, hence the precedence of the reference's checks) and the tally must equal the oracle's."""
    if workload == "single":
        p = eg.ChoiceParams(ctx, pk, 5, True); op = oracle.ChoiceParams(pk, 5, True); kw = {}
    elif workload == "multi":
        p = eg.ChoiceParams(ctx, pk, 6, False); op = oracle.ChoiceParams(pk, 6, False); kw = {"n_selected": 2}
    else:
        p = eg.QuadraticVotingParams(ctx, pk, 4, 12); op = oracle.QvParams(pk, 4, 12); kw = {}
    n = 3000 if workload != "qv" else 1200
    import torch

    sz = p.ballot_size
    d = torch.empty(n * sz, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(4242, 0, n, d.data_ptr(), **kw)
    ctx.synchronize()
    ballots = bytearray(d.cpu().numpy().tobytes())
    rnd = random.Random(99)
    for b in range(n):
        if b % 10 == 0:
            continue                                   # every tenth ballot stays valid
        for _ in range(rnd.randrange(1, 4)):
            ballots[b * sz + rnd.randrange(sz)] ^= 1 << rnd.randrange(8)
    want = op.verify_batch(bytes(ballots), threads=8)
    got, tally = p.verify_batch(bytes(ballots))
    assert got == want
    assert tally == op.tally(bytes(ballots), want)
    kinds = {w & 0xFF for w in want}
    assert 0 in kinds and len(kinds) >= 4              # accepted, bad scalar, bad point and at least one proof failure


def test_chunks_shrink_when_device_memory_is_taken(eg, ctx, oracle, pk):
    """The chunk workspace is sized from the memory free at params creation; if another allocation takes that memory
    before the first big batch, the engine must fall back to smaller chunks instead of failing."""
    import torch

    p = eg.ChoiceParams.single_choice(ctx, pk, 5)
    op = oracle.ChoiceParams(pk, 5, True)
    n = 400_000
    sz = p.ballot_size
    d = torch.empty(n * sz, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(5150, 0, n, d.data_ptr())
    ctx.synchronize()
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    hog = torch.empty(max(free - (18 << 30), 1 << 20), dtype=torch.uint8, device="cuda")   # leave ~18 GB: 400k ballots need ~23 GB
    try:
        p.tally_reset()
        p.verify_batch_device(n, d.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0
        tally = p.tally_encode()
    finally:
        del hog
        torch.cuda.empty_cache()
    head = bytes(d[: 64 * sz].cpu().numpy())
    assert st[:64].tolist() == op.verify_batch(head)
    # tally of the whole batch = tally of two halves verified with ample memory
    p2 = eg.ChoiceParams.single_choice(ctx, pk, 5)
    p2.tally_reset()
    p2.verify_batch_device(n, d.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert p2.tally_encode() == tally


# ------------------------------------------------------------------ object ingest: length-mismatch verdicts
@pytest.mark.parametrize("kind", ["single", "multi", "qv"])
def test_object_ingest_length_mismatches(eg, ctx, oracle, pk, kind):
    """Ballots as serde-layout objects with wrong numbers of choices / responses / partial ciphertexts: the verdicts follow
    the reference's order of checks (tests/ingest_cases.py; the same scenarios run oracle-backed in test_ingest_cpu.py)."""
    from elastic_elgamal_amd import ingest, serde
    from ingest_cases import choice_cases, qv_cases

    grp = eg.Ristretto(ctx)
    if kind == "qv":
        n, credits = 3, 9
        op = oracle.QvParams(pk, n, credits)
        p = eg.QuadraticVotingParams(ctx, pk, n, credits)
        packed = op.generate_batch(12, 0, 8)
        sz = len(packed) // 8
        cases = qv_cases([ingest.unpack_qv_ballot(packed[i * sz : (i + 1) * sz], n, credits) for i in range(8)])
        got, tally = ingest.verify_qv_objects(p, grp, [c[1] for c in cases])
        accepted = b"".join(serde.pack_qv_ballot(c[1]) for c in cases if c[2] == 0)
    else:
        n, single = 3, kind == "single"
        op = oracle.ChoiceParams(pk, n, single)
        p = eg.ChoiceParams(ctx, pk, n, single)
        packed = op.generate_batch(11, 0, 8, n_selected=0 if single else 2)
        sz = len(packed) // 8
        cases = choice_cases([serde.unpack_encrypted_choice(packed[i * sz : (i + 1) * sz], n, single) for i in range(8)], single)
        got, tally = ingest.verify_choice_objects(p, grp, [c[1] for c in cases])
        accepted = b"".join(serde.pack_encrypted_choice(c[1]) for c in cases if c[2] == 0)
    for (name, _, want), g in zip(cases, got):
        assert g == want, name
    assert tally == op.tally(accepted, [0] * (len(accepted) // sz))


@pytest.mark.parametrize("kind", ["single", "qv"])
def test_json_text_ingest_matches_object_path(eg, ctx, oracle, pk, kind):
    """Ballots as JSON text (serde's layout): native packer + one GPU batch for the well-shaped ones, the object path for the
    rest; verdicts and tally must equal those of the object path on the parsed objects (which the oracle-backed CPU tests pin)."""
    import json
    from elastic_elgamal_amd import ingest, serde
    from ingest_cases import choice_cases, qv_cases

    grp = eg.Ristretto(ctx)
    if kind == "qv":
        n, credits = 3, 9
        op = oracle.QvParams(pk, n, credits)
        p = eg.QuadraticVotingParams(ctx, pk, n, credits)
        packed = op.generate_batch(21, 0, 200, threads=8)
        sz = len(packed) // 200
        objs = [ingest.unpack_qv_ballot(packed[i * sz : (i + 1) * sz], n, credits) for i in range(200)]
        cases = [c[1] for c in qv_cases(objs[:8])]
        verify_objects, verify_json = ingest.verify_qv_objects, ingest.verify_qv_json
    else:
        n = 3
        op = oracle.ChoiceParams(pk, n, True)
        p = eg.ChoiceParams(ctx, pk, n, True)
        packed = op.generate_batch(22, 0, 200, threads=8)
        sz = len(packed) // 200
        objs = [serde.unpack_encrypted_choice(packed[i * sz : (i + 1) * sz], n, True) for i in range(200)]
        cases = [c[1] for c in choice_cases(objs[:8], True)]
        verify_objects, verify_json = ingest.verify_choice_objects, ingest.verify_choice_json
    batch = objs[8:100] + cases + objs[100:]
    batch[5] = dict(batch[5]); batch[5].pop(next(iter(batch[5])))                    # a missing field: Malformed
    want, want_tally = verify_objects(p, grp, batch)
    for text in (json.dumps(batch), "\n".join(json.dumps(o, indent=1) for o in batch)):
        got, tally = verify_json(p, grp, text)
        assert got == want and tally == want_tally
    assert want.count(0) >= 190 and eg.MALFORMED in want and len({w & 0xFF for w in want}) >= 4


@pytest.mark.parametrize("kind", ["single", "qv"])
def test_native_json_verify_entry(eg, ctx, oracle, pk, kind):
    """eg_verify_*_json: JSON text -> verdicts + tally inside the library (host threads pack piece k+1 while the GPU verifies
    piece k).  Objects whose shape is not the election's get the reference's verdict below the C ABI (OptionsLenMismatch /
    LenMismatch in verify()'s order, csrc/wire_json.hpp: resolve_*_objects): every verdict equals the Python object path's
    (ingest.verify_*_objects, pinned by oracle/objects.c in the CPU tests) and the scenario table's expectation; the tally is the
    call's own and the running tally accumulates; several pieces (300 000 objects) agree with the packed path."""
    import json
    from elastic_elgamal_amd import ingest, serde
    from ingest_cases import choice_cases, qv_cases

    grp = eg.Ristretto(ctx)
    if kind == "qv":
        n, credits = 3, 9
        op = oracle.QvParams(pk, n, credits)
        p = eg.QuadraticVotingParams(ctx, pk, n, credits)
        packed = op.generate_batch(21, 0, 64, threads=8)
        sz = len(packed) // 64
        objs = [ingest.unpack_qv_ballot(packed[i * sz : (i + 1) * sz], n, credits) for i in range(64)]
        table = qv_cases(objs[:8])
        recipe = ingest.verify_qv_objects
    else:
        n = 3
        op = oracle.ChoiceParams(pk, n, True)
        p = eg.ChoiceParams(ctx, pk, n, True)
        packed = op.generate_batch(22, 0, 64, threads=8)
        sz = len(packed) // 64
        objs = [serde.unpack_encrypted_choice(packed[i * sz : (i + 1) * sz], n, True) for i in range(64)]
        table = choice_cases(objs[:8], True)
    cases = [c[1] for c in table]
    if kind == "single":
        recipe = ingest.verify_choice_objects
    batch = objs[8:30] + cases + [{"votes": 1, "choices": 2}] + objs[30:]
    text = json.dumps(batch)
    want, want_tally = recipe(p, grp, batch)          # the Python object path on the parsed objects (pinned by oracle/objects.c on the CPU)
    p.tally_reset()
    got, tally = p.verify_json(text)
    packer_status = eg.pack_json(text, n, single=True)[1] if kind == "single" else eg.pack_json(text, n, credits=credits)[1]
    assert len(got) == len(want) == len(batch)
    assert got == want                                                   # reshaped objects included
    assert got[22 : 22 + len(table)] == [c[2] for c in table], [c[0] for c, g in zip(table, got[22:]) if c[2] != g]
    assert tally == want_tally == p.tally_encode()
    assert eg.MALFORMED in got and eg.PACK_RESHAPE in packer_status and eg.PACK_RESHAPE not in got and got.count(0) >= 50
    # the multi-choice election has no sum proof: a reshaped ballot is Range(LenMismatch) straight away (choice.rs:370-379)
    if kind == "single":
        om = oracle.ChoiceParams(pk, n, False)
        pm = eg.ChoiceParams(ctx, pk, n, False)
        mp = om.generate_batch(23, 0, 8, n_selected=2)
        msz = len(mp) // 8
        mt = choice_cases([serde.unpack_encrypted_choice(mp[i * msz : (i + 1) * msz], n, False) for i in range(8)], False)
        got_m, _ = pm.verify_json(json.dumps([c[1] for c in mt]))
        assert got_m == [c[2] for c in mt], [c[0] for c, g in zip(mt, got_m) if c[2] != g]
    if kind == "single":        # many pieces: 300 000 ballots from the GPU prover as one JSON array
        import torch
        m = 300_000
        d = torch.empty(m * sz, dtype=torch.uint8, device="cuda")
        p.encrypt_batch_device(99, 0, m, d.data_ptr())
        ctx.synchronize()
        raw = bytearray(d.cpu().numpy().tobytes())
        for i in range(0, m, 1000):
            raw[i * sz + sz - 32] ^= 1                       # every 1000th ballot tampered
        raw = bytes(raw)
        big = "[" + ",".join(json.dumps(serde.unpack_encrypted_choice(raw[i * sz : (i + 1) * sz], n, True)) for i in range(m)) + "]"
        want_st, want_t = p.verify_batch(raw)
        got_st, got_t = p.verify_json(big, max_objects=m)
        assert got_st == want_st and got_t == want_t and got_st.count(0) == m - 300


@pytest.mark.parametrize("ring_kb,window_kb,streams", [(100, 16, 2), (64, 200, 2), (900, 40, 2), (100, 16, 1)])
def test_json_pipeline_ring_wraps_and_small_windows(eg, ctx, oracle, pk, monkeypatch, ring_kb, window_kb, streams):
    """The streaming pipeline of eg_verify_*_json with a pinned ring far smaller than the text (test knobs EG_JSON_RING_KB /
    EG_JSON_WINDOW_KB): windows of a dozen ballots, a ring that wraps hundreds of times, the producer waiting for the GPU and the GPU
    for the producer; with two work sets (submissions overlap on two control streams) and with one (EG_STREAMS=1: one after the other).
    Verdicts (tampered, junk and reshaped objects among them), the call's tally and the running tally must equal the packed path's."""
    import json
    import torch
    from elastic_elgamal_amd import serde
    n, m = 3, 6000
    monkeypatch.setenv("EG_STREAMS", str(streams))          # read when the params object is made
    p = eg.ChoiceParams(ctx, pk, n, True)
    sz = p.ballot_size
    d = torch.empty(m * sz, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(77, 0, m, d.data_ptr())
    ctx.synchronize()
    raw = bytearray(d.cpu().numpy().tobytes())
    for i in range(0, m, 97):
        raw[i * sz + sz - 32] ^= 1
    raw = bytes(raw)
    objs = [serde.unpack_encrypted_choice(raw[i * sz : (i + 1) * sz], n, True) for i in range(m)]
    short = dict(objs[5]); short["choices"] = short["choices"][:2]          # another shape: OptionsLenMismatch through the object path
    texts = [json.dumps(o) for o in objs]
    texts[1234] = '{"junk": [1, 2, {"a": "}"}]}'
    texts[4321] = json.dumps(short)
    big = "[" + ",\n".join(texts) + "]"
    p.tally_reset()
    want_st, want_t = p.verify_json(big, max_objects=m)                   # default windows: one region
    assert want_st[1234] == eg.MALFORMED and want_st[4321] not in (0, eg.MALFORMED) and want_st.count(0) == m - len(range(0, m, 97)) - 2
    ref_st, _ = p.verify_batch(raw)
    assert [a for i, a in enumerate(ref_st) if i not in (1234, 4321)] == [a for i, a in enumerate(want_st) if i not in (1234, 4321)]
    monkeypatch.setenv("EG_JSON_RING_KB", str(ring_kb))                    # read when a params object is made: a second one, same election
    monkeypatch.setenv("EG_JSON_WINDOW_KB", str(window_kb))
    p.close()
    p = eg.ChoiceParams(ctx, pk, n, True)
    got_st, got_t = p.verify_json(big, max_objects=m)
    assert got_st == want_st and got_t == want_t == p.tally_encode()
    got2, t2 = p.verify_json(big, max_objects=m)                          # the running tally keeps accumulating, the call's tally is its own
    assert got2 == want_st and t2 == want_t and p.tally_encode() != want_t
    with pytest.raises(eg.EgError):
        p.verify_json(big, max_objects=m - 1)                             # more objects than the caller made room for
    with pytest.raises(eg.EgError):
        p.verify_json(big[: len(big) // 2], max_objects=m)                # a truncated text fails as a whole
    p.tally_reset()
    assert p.verify_json(big, max_objects=m) == (want_st, want_t)          # and the engine is in order afterwards


@pytest.mark.parametrize("kind", ["single", "qv"])
def test_json_stream_equals_the_one_shot_entry(eg, ctx, oracle, pk, kind, monkeypatch):
    """eg_verify_*_json_begin / eg_verify_json_feed / _take / _end (VERDICT r4 task 7; examples/voting.rs:195-198 prints ballots one at a
    time, src/serde.rs:19-80): the text fed in pieces - one byte at a time, random sizes, one piece - gives the verdicts and the tally of
    eg_verify_*_json on the whole text: tampered ballots, junk objects, objects of another shape (object path at the end), escaped
    strings, with a staging ring far smaller than the text (it wraps; feed waits for the GPU).  take() hands out final verdicts in
    order and never one that is still open; the params object refuses other calls while a stream is open; abort and a failed feed
    leave the running tally as it was; the running tally has a finished stream's ballots added."""
    import json
    from elastic_elgamal_amd import ingest, serde
    from ingest_cases import choice_cases, qv_cases

    rnd = random.Random(4711)
    if kind == "qv":
        n, credits, m = 3, 9, 700
        op = oracle.QvParams(pk, n, credits)
        mk = lambda: eg.QuadraticVotingParams(ctx, pk, n, credits)
        packed = bytearray(op.generate_batch(61, 0, m, threads=8))
        sz = len(packed) // m
        unpack = lambda b: ingest.unpack_qv_ballot(b, n, credits)
        cases = lambda objs: qv_cases(objs)
    else:
        n, m = 3, 1500
        op = oracle.ChoiceParams(pk, n, True)
        mk = lambda: eg.ChoiceParams(ctx, pk, n, True)
        packed = bytearray(op.generate_batch(62, 0, m, threads=8))
        sz = len(packed) // m
        unpack = lambda b: serde.unpack_encrypted_choice(b, n, True)
        cases = lambda objs: choice_cases(objs, True)
    for i in range(0, m, 37):
        packed[i * sz + sz - 32] ^= 1
    objs = [unpack(bytes(packed[i * sz : (i + 1) * sz])) for i in range(m)]
    table = [c[1] for c in cases(objs[:8])]
    batch = objs[8:400] + table + [{"junk": ["}", "]", "\\\"", {"a": "{"}]}, {"votes": 1, "choices": 2}] + objs[400:]
    texts = [json.dumps(o) for o in batch]
    for whole in ("[" + ",".join(texts) + "]", "\n".join(texts) + "\n", " [ " + " ,\n ".join(texts) + " ]\n\n"):
        p = mk()
        want, want_tally = p.verify_json(whole)
        assert len(want) == len(batch) and eg.MALFORMED in want and want.count(0) > m // 2
        p.close()
        data = whole.encode()
        plans = [[len(data)], None, "bytes"] if whole.startswith("[") else [None]
        for plan in plans:
            for ring_kb in (0, 48):
                if plan == "bytes" and (ring_kb or kind == "qv"):
                    continue
                if ring_kb:
                    monkeypatch.setenv("EG_JSON_RING_KB", str(ring_kb))
                    monkeypatch.setenv("EG_JSON_WINDOW_KB", "8")
                p = mk()
                monkeypatch.delenv("EG_JSON_RING_KB", raising=False)
                monkeypatch.delenv("EG_JSON_WINDOW_KB", raising=False)
                st = p.json_stream(threads=4)
                with pytest.raises(eg.EgError, match="stream is open"):
                    p.verify_batch(bytes(packed[:sz]))
                with pytest.raises(eg.EgError, match="stream is open"):
                    p.tally_encode()
                with pytest.raises(eg.EgError, match="already open"):
                    p.json_stream()
                got, at = [], 0
                if plan == "bytes":
                    sizes = [1] * 5000 + [len(data) - 5000]
                elif plan is None:
                    sizes = []
                    while sum(sizes) < len(data):
                        sizes.append(min(rnd.choice((1, 7, 100, 1000, 5000, 40000, 300000)), len(data) - sum(sizes)))
                else:
                    sizes = plan
                for k, size in enumerate(sizes):
                    seen = st.feed(data[at : at + size])             # objects the stream's worker has cut so far (it may lag behind the feeds)
                    at += size
                    assert seen <= len(batch)
                    if k % 5 == 0:
                        got += st.take(1000)
                        assert len(got) <= len(batch)
                assert at == len(data)
                rest, tally = st.end()
                got += rest
                assert st.objects == len(batch)
                assert got == want, (plan if plan != "bytes" else "bytes", ring_kb, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:5])
                assert tally == want_tally == p.tally_encode()                    # the running tally has the stream's ballots
                # a second stream on the same object: aborted half way, the running tally stays; then one that fails in the text
                st = p.json_stream(threads=2)
                st.feed(data[: len(data) // 2])
                st.abort()
                assert p.tally_encode() == want_tally
                st = p.json_stream(threads=2)
                cut = data.index(texts[100].encode()) + len(texts[100].encode())       # right after a complete ballot
                st.feed(data[:cut])
                # small pieces are only copied by feed (a worker thread cuts them): the error of the text shows at a later feed, at
                # take, or at the latest at end - which reports it and cleans up
                with pytest.raises(eg.EgError, match="neither a JSON array|closing bracket"):
                    st.feed(b"] ] garbage")
                    for _ in range(2000):
                        st.feed(b" ")
                        st.take(1)
                    st.end()
                if st._h:                                                          # reported by a feed / take: the stream is dead, end cleans up
                    with pytest.raises(eg.EgError):
                        st.feed(b"{}")
                    with pytest.raises(eg.EgError, match="neither a JSON array|closing bracket"):
                        st.end()
                assert not st._h
                assert p.tally_encode() == want_tally
                st = p.json_stream(threads=2)                                      # a truncated text fails at the end
                st.feed(data[: len(data) - 40])
                with pytest.raises(eg.EgError, match="ends inside a value|never closes|separator"):
                    st.end()
                assert p.tally_encode() == want_tally
                got2, t2 = p.verify_json(whole)                                     # and the object is in order afterwards
                assert got2 == want and t2 == want_tally
                p.close()
    p = mk()                                            # an empty text, and a params object destroyed with a stream open
    st = p.json_stream()
    assert st.end() == ([], bytes(64 * n))
    st = p.json_stream()
    st.feed(b"[")
    p.close()                                           # the params object takes the open stream with it (and the Python handle is cleared)
    assert not st._h


def test_json_stream_one_million_ballots_in_one_megabyte_pieces(eg, ctx, pk):
    """VERDICT r4 task 7 'done': 1 M single-choice ballots (every 1000th tampered) as one JSON array fed in 1 MB pieces equal the one-shot
    entry on the same text - verdicts and tally - and the packed path."""
    import ctypes as C
    import json

    import numpy as np
    import torch
    from elastic_elgamal_amd import serde

    n, m, distinct = 5, 1_000_000, 2000
    p = eg.ChoiceParams(ctx, pk, n, True)
    sz = p.ballot_size
    d = torch.empty(distinct * sz, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(4321, 0, distinct, d.data_ptr())
    ctx.synchronize()
    raw = bytearray(d.cpu().numpy().tobytes())
    for i in range(0, distinct, 1000):
        raw[i * sz + sz - 32] ^= 1
    raw = bytes(raw)
    one = [json.dumps(serde.unpack_encrypted_choice(raw[i * sz : (i + 1) * sz], n, True)) for i in range(distinct)]
    text = ("[" + ",".join(one * (m // distinct)) + "]").encode()
    want = (C.c_uint32 * m)()
    p.tally_reset()
    assert p.verify_json_into(text, want, 16) == m
    want_tally = p.tally_encode()
    p.tally_reset()
    st = p.json_stream(threads=16)
    base = C.cast(C.c_char_p(text), C.c_void_p).value
    for at in range(0, len(text), 1 << 20):
        st.feed_ptr(base + at, min(1 << 20, len(text) - at))
    got = (C.c_uint32 * m)()
    taken, tally = st.end_into(got, with_tally=True)
    assert taken == m and st.objects == m
    g, w = np.frombuffer(got, dtype=np.uint32), np.frombuffer(want, dtype=np.uint32)
    assert np.array_equal(g, w) and int((g == 0).sum()) == m - m // 1000
    assert tally == want_tally == p.tally_encode()
    ref_st, ref_t = p.verify_batch(raw)
    assert list(g[:distinct]) == ref_st
    p.close()


@pytest.mark.parametrize("upper_bound", [12, 15, 20, 50])
def test_range_proof_negative_cases(eg, ctx, oracle, pk, upper_bound):
    """range.rs:708-795 (range_proof_basics): a proof must not verify for another receiver, another ciphertext, a mangled
    ciphertext or another decomposition; every verdict equals the oracle's."""
    grp = eg.Ristretto(ctx)
    k = oracle.PublicKey(pk)
    pr = oracle.PreparedRange(upper_bound)
    rs = oracle.rng_from_u64(1000 + upper_bound)
    a, b = k.encrypt_range(pr, 10, rs), k.encrypt_range(pr, 3, rs)
    r = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.RANGE, upper_bound)
    gen = oracle.point_mul_generator(sc(1))
    mangled_b, _ = grp.element_add(a[32:64], gen)                     # blinded_element += G
    cases = [a, b,
             b[:64] + a[64:],                                         # another ciphertext under a's proof
             a[:32] + mangled_b + a[64:],                             # mangled ciphertext
             a[:64] + b[64:]]                                         # a's ciphertext under another proof
    want = [k.verify_range(pr, c) for c in cases]
    assert want[:2] == [0, 0] and all(w != 0 for w in want[2:])
    assert r.verify_batch(b"".join(cases)) == want
    # another receiver
    pk2 = oracle.point_mul_generator(sc(123456789))
    r2 = eg.PublicKeyVerifier(ctx, pk2, eg.PublicKeyVerifier.RANGE, upper_bound)
    k2 = oracle.PublicKey(pk2)
    assert r2.verify_batch(a + b) == [k2.verify_range(pr, a), k2.verify_range(pr, b)] != [0, 0]
    # another decomposition of the same wire size, where one exists among nearby bounds
    for other in range(upper_bound + 1, upper_bound + 40):
        pro = oracle.PreparedRange(other)
        if pro.proof_size == pr.proof_size and eg.range_decomposition(other) != eg.range_decomposition(upper_bound):
            ro = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.RANGE, other)
            got = ro.verify_batch(a + b)
            assert got == [k.verify_range(pro, a), k.verify_range(pro, b)] and all(x != 0 for x in got)
            break


def test_qv_reordered_votes(eg, ctx, oracle, pk):
    """mul.rs:332-361 (reordering the ciphertexts breaks the sum-of-squares proof): swapping two vote blocks keeps every
    range proof valid, so the failure must be CreditEquivalence."""
    n, credits = 4, 16
    oq = oracle.QvParams(pk, n, credits)
    q = eg.QuadraticVotingParams(ctx, pk, n, credits)
    ballots = bytearray(oq.generate_batch(41, 0, 40, threads=8))
    sz = q.ballot_size
    from elastic_elgamal_amd import ingest
    rings = ingest.parse_range(eg.range_decomposition(ingest.isqrt(credits) + 1))
    vote_sz = 64 + 64 * (len(rings) - 1) + 32 * (1 + sum(s for _, s in rings))
    for b in range(0, 40, 2):
        o = b * sz
        v0, v1 = bytes(ballots[o : o + vote_sz]), bytes(ballots[o + vote_sz : o + 2 * vote_sz])
        ballots[o : o + vote_sz], ballots[o + vote_sz : o + 2 * vote_sz] = v1, v0
    want = oq.verify_batch(bytes(ballots), threads=8)
    got, tally = q.verify_batch(bytes(ballots))
    assert got == want and tally == oq.tally(bytes(ballots), want)
    kinds = {w & 0xFF for w in want[0:40:2]}
    assert kinds == {12}                                        # CREDIT_EQUIV_CHALLENGE


def test_tally_checkpoint_and_resume(eg, ctx, oracle, pk):
    """SURVEY 5 (checkpoint / resume): a running tally exported with tally_encode and re-imported with tally_add into a
    fresh params object continues exactly; invalid encodings are refused."""
    op = oracle.ChoiceParams(pk, 5, True)
    ballots = bytearray(op.generate_batch(77, 0, 200, threads=8))
    sz = len(ballots) // 200
    ballots[3 * sz + sz - 32] ^= 1
    want = op.verify_batch(bytes(ballots), threads=8)
    whole = op.tally(bytes(ballots), want)
    a = eg.ChoiceParams.single_choice(ctx, pk, 5)
    st_a, checkpoint = a.verify_batch(bytes(ballots[: 120 * sz]))
    b = eg.ChoiceParams.single_choice(ctx, pk, 5)           # "another process": resumes from the checkpoint bytes
    b.tally_reset()
    b.tally_add(checkpoint)
    import torch
    d = torch.frombuffer(bytearray(ballots[120 * sz :]), dtype=torch.uint8).cuda()
    st = torch.empty(80, dtype=torch.int32, device="cuda")
    b.verify_batch_device(80, d.data_ptr(), st.data_ptr())
    assert st_a + st.cpu().tolist() == want
    assert b.tally_encode() == whole
    with pytest.raises(Exception):
        b.tally_add(b"\xff" * (64 * 5))
    assert b.tally_encode() == whole                         # untouched by the refused import


def test_host_form_accumulates_and_reports_its_own_batch(eg, ctx, oracle, pk):
    """eg_hip.h tally semantics: every verify call (host or device form) adds to the running tally; tally_out of the host
    form is the tally of that call's batch alone.  A checkpoint restored with tally_add must survive a host verify_batch."""
    op = oracle.ChoiceParams(pk, 5, True)
    ballots = bytearray(op.generate_batch(4711, 0, 90, threads=8))
    sz = len(ballots) // 90
    ballots[50 * sz + sz - 32] ^= 1
    ballots = bytes(ballots)
    want = op.verify_batch(ballots, threads=8)
    t_all = op.tally(ballots, want)
    parts = [ballots[: 30 * sz], ballots[30 * sz : 60 * sz], ballots[60 * sz :]]
    t_parts = [op.tally(b, want[30 * i : 30 * i + 30]) for i, b in enumerate(parts)]
    p = eg.ChoiceParams.single_choice(ctx, pk, 5)
    p.tally_reset()
    p.tally_add(t_parts[0])                                  # restored checkpoint: the first 30 ballots were verified elsewhere
    st1, own1 = p.verify_batch(parts[1])                     # host form WITH tally_out
    assert st1 == want[30:60] and own1 == t_parts[1]         # its own batch only ...
    grp = eg.Ristretto(ctx)
    assert p.tally_encode() == grp.element_add(t_parts[0], t_parts[1])[0]    # ... and the running tally kept the checkpoint
    st2, none = p.verify_batch(parts[2], with_tally=False)   # host form WITHOUT tally_out accumulates as well
    assert st2 == want[60:] and none is None
    assert p.tally_encode() == t_all
    st3, own3 = p.verify_batch(b"")                          # an empty batch: identity tally, running tally untouched
    assert st3 == [] and own3 == bytes(320) and p.tally_encode() == t_all
    p.tally_reset()
    assert p.tally_encode() == bytes(320)


def test_points_sum_flags_undecodable_tallies(eg, ctx, oracle, pk):
    """eg_points_sum_device: an all-gathered tally that does not decode must be reported, not silently dropped."""
    import torch

    op = oracle.ChoiceParams(pk, 5, True)
    ballots = op.generate_batch(31, 0, 8)
    t = op.tally(ballots, [0] * 8)
    two = torch.frombuffer(bytearray(t + t), dtype=torch.uint8).cuda()
    out = torch.empty(320, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.points_sum_device(2, 10, two.data_ptr(), out.data_ptr(), d_bad=bad.data_ptr())
    ctx.synchronize()
    assert int(bad.item()) == 0
    assert bytes(out.cpu().numpy()) == eg.Ristretto(ctx).element_add(t, t)[0]
    two[320 + 64 : 320 + 96] = 0xFF                          # rank 1's third point is garbage
    ctx.points_sum_device(2, 10, two.data_ptr(), out.data_ptr(), d_bad=bad.data_ptr())
    ctx.synchronize()
    assert int(bad.item()) == 1


# ------------------------------------------------------------------ the RCCL leg and the fixed-total mode of bench.py
def _run_bench(*args, timeout=600):
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29600 + os.getpid() % 300), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(root / "bench.py"), *args], capture_output=True, text=True, timeout=timeout, env=env,
                       cwd=str(root))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_rccl_leg_in_a_fresh_process():
    """The N > 1 code path of bench.py on the one GPU of the box: torch.distributed over RCCL is initialised for a single
    rank, the tally goes through tally_encode_device -> all_gather_into_tensor -> eg_points_sum_device on the shared stream,
    and must come out equal to the engine's own tally (examples/voting.rs:199-203 is what the exchange stands in for)."""
    line = _run_bench("--full", "--gpus", "1", "--force-dist", "--ballots", "131072", "--steps", "1", "--warmup", "0", "--no-cpu-baseline")
    assert line["config"]["tally_exchange_ok"] is True
    assert line["config"]["accepted"] == 131072 and line["n_gpus"] == 1 and line["scaling"] == "weak"
    assert line["roofline"]["frac"] > 0 and line["value"] > 1e5
    assert line["host_inclusive"]["verdicts_match_device_path"] is True


@pytest.mark.parametrize("mode", ["weak", "strong"])
def test_bench_two_ranks_rehearsed_on_one_gpu(mode):
    """bench.py itself with N = 2, launched the way the driver launches it (python -m torch.distributed.run, one JSON line from rank 0):
    both ranks use the one GPU of the box and exchange through gloo (--rehearse-one-gpu), so the value means nothing, but every line of the
    multi-rank path runs - sharding, barriers, max over ranks, the tally all-gather and its check on every rank, the extra isolated step,
    rank 0 alone printing.  weak: 60 000 ballots per rank; strong: 100 001 ballots split 50 000 / 50 001 (BASELINE configs[4] in small)."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    size = ["--ballots", "60000"] if mode == "weak" else ["--total-ballots", "100001"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(29700 + os.getpid() % 200), str(root / "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--rehearse-one-gpu", "--tampered-percent", "1", "--selfbench-seconds", "0.5", "--cpu-seconds", "2", *size]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(root))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines                                     # rank 0 alone prints, ONE line
    line = json.loads(lines[0])
    total = 120000 if mode == "weak" else 100001
    assert line["n_gpus"] == 2 and line["scaling"] == mode and line["config"]["total_ballots"] == total
    assert line["config"]["tally_exchange_ok"] is True
    assert line["config"]["accepted"] == total - line["config"]["tampered"] and line["config"]["tampered"] > 0
    assert line["config"]["parallelism"] == "shard2" and line["value"] > 1e4 and line["roofline"]["isolated"]["frac"] > 0
    # a scaling line that explains itself (VERDICT r5 task 1): every rank's own step time, clock and verdict count, the exchange timed on
    # its own, the CPU baseline at N > 1, and the PCIe-inclusive and JSON legs on EVERY rank at the same time
    pr = line["per_rank"]
    assert [r["rank"] for r in pr] == [0, 1] and all(r["ms_per_step"] > 0 and r["device"] == 0 for r in pr)
    assert sum(r["accepted"] for r in pr) == line["config"]["accepted"] and line["slowest_rank"] in (0, 1)
    assert line["exchange"]["us_per_step"] > 0 and line["exchange"]["bytes_per_rank"] == 320
    assert line["cpu_baseline"]["verdicts_match_gpu"] is True and line["cpu_baseline"]["cores"] >= 1
    hi = line["host_inclusive"]["all_ranks"]
    assert hi["ranks"] == 2 and hi["verdicts_match_device_path"] is True and hi["sum_value"] >= hi["max_value"] > 0
    assert all(r["host_inclusive_ok"] and r["host_inclusive_value"] > 0 for r in pr)
    js = line["json_inclusive"]["all_ranks"]
    assert js["ranks"] == 2 and js["verdicts_match_device_path"] is True and js["sum_value"] > 0 and js["threads_per_rank"] >= 1
    assert 100 < line["valu_roofline"]["box"]["fmul_sustained_g"] < 320 and all(r["fmul_box_g"] > 0 for r in pr)      # (two ranks share the GPU here)


def test_two_ranks_real_gpu_tallies(eg, ctx, pk, tmp_path):
    """N = 2 with REAL GPU tallies (BASELINE configs[4] in small): two fresh child processes, each initialising the GPU itself (both on
    device 0), form a gloo group; each verifies its shard_range slab of one 200 000-ballot batch (1 % tampered) with the HIP engine,
    the tallies are exchanged with gather_tallies and merged with eg_points_sum_device (d_bad == 0).  Both ranks must hold the
    tally and the accepted count of a single-process run over the whole batch (examples/voting.rs:199-203)."""
    import json
    import os
    import subprocess
    import sys
    import time
    from pathlib import Path

    import torch

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from dist_gpu_worker import tamper

    total, seed, world = 200_000, 424242, 2
    port = 29900 + os.getpid() % 90
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    # the whole batch in THIS process first (its GPU runtime is up before the children start theirs)
    p = eg.ChoiceParams.single_choice(ctx, pk, 5)
    d = torch.empty(total * p.ballot_size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(seed, 0, total, d.data_ptr())
    ctx.synchronize()
    assert tamper(d.view(total, p.ballot_size), 0, total) == total // 100
    st = torch.empty(total, dtype=torch.int32, device="cuda")
    p.tally_reset()
    p.verify_batch_device(total, d.data_ptr(), st.data_ptr())
    want_tally = p.tally_encode()
    want_accepted = int((st == 0).sum())
    assert want_accepted == total - total // 100
    worker = str(Path(__file__).resolve().parent / "dist_gpu_worker.py")
    del d, st
    torch.cuda.empty_cache()
    procs = []
    for r in range(world):
        procs.append(subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), str(total), str(seed),
                                       str(tmp_path / f"r{r}.json")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        time.sleep(2.0)          # the ranks bring up their GPU runtimes one after the other (they meet in the gloo rendezvous anyway)
    for pr in procs:
        text, _ = pr.communicate(timeout=600)
        assert pr.returncode == 0, text[-3000:]
    res = sorted((json.loads((tmp_path / f"r{r}.json").read_text()) for r in range(world)), key=lambda x: x["rank"])
    assert [tuple(r["range"]) for r in res] == [(0, total // 2), (total // 2, total)]
    for r in res:
        assert r["d_bad"] == 0
        assert r["accepted"] == want_accepted
        assert bytes.fromhex(r["merged"]) == want_tally              # sharding and the exchange do not change the tally
    assert res[0]["local"] != res[1]["local"]                          # the shards really differ
    assert res[0]["accepted_local"] + res[1]["accepted_local"] == want_accepted


def test_bench_fixed_total_mode():
    """`--total-ballots N` (BASELINE.json configs[4]: a fixed batch sharded over the ranks) with 1 % tampered ballots."""
    line = _run_bench("--full", "--gpus", "1", "--total-ballots", "300000", "--tampered-percent", "1", "--steps", "1", "--warmup", "0",
                      "--no-cpu-baseline", "--no-host-inclusive")
    assert line["scaling"] == "strong" and line["config"]["total_ballots"] == 300000
    assert line["config"]["accepted"] == 300000 - 3000 and line["config"]["tally_exchange_ok"] is True


def test_bench_plain_run_dumps_what_its_last_step_computed(oracle, pk, tmp_path):
    """Without --full bench.py prints the headline line alone; --dump-outputs writes the verdict words and the exchanged tally of the last
    timed step, which must be the oracle's on the same seeded ballots (1 % tampered, as bench.py tampers them).  The in-process path's
    dump and the primitive tier's products are checked against the oracle the same way."""
    import numpy as np
    import torch

    n, seed = 4096, 20260612
    line = _run_bench("--gpus", "1", "--ballots", str(n), "--tampered-percent", "1", "--steps", "3", "--warmup", "1",
                      "--dump-outputs", str(tmp_path / "single"))
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "ballots/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u32"
    assert not {"roofline", "valu_roofline", "cpu_baseline", "host_inclusive", "wire_ingest", "extra"} & set(line)
    op = oracle.ChoiceParams(pk, 5, True)
    ballots = bytearray(op.generate_batch(seed, 0, n, threads=8))
    bad = torch.randperm(n, generator=torch.Generator(device="cpu").manual_seed(seed))[: n // 100].tolist()
    for i in bad:
        ballots[(i + 1) * op.ballot_size - 32] ^= 1
    want = op.verify_batch(bytes(ballots), threads=8)
    status = np.load(tmp_path / "single" / "status.npy")
    tally = np.load(tmp_path / "single" / "tally.npy")
    assert status.dtype == np.float64 and status.tolist() == want and sorted(np.flatnonzero(status).tolist()) == sorted(bad)
    assert bytes(tally.astype(np.uint8)) == op.tally(bytes(ballots), want)

    _run_bench("--in-process-devices", "2", "--rehearse-one-gpu", "--ballots", str(n // 2), "--steps", "2", "--warmup", "1",
               "--dump-outputs", str(tmp_path / "in_process"))
    clean = op.generate_batch(seed, 0, n, threads=8)
    assert not np.load(tmp_path / "in_process" / "status.npy").any()
    assert bytes(np.load(tmp_path / "in_process" / "tally.npy").astype(np.uint8)) == op.tally(clean, [0] * n)

    line = _run_bench("--gpus", "1", "--workload", "msm", "--ballots", "2048", "--steps", "1", "--warmup", "1",
                      "--dump-outputs", str(tmp_path / "msm"))
    assert line["steps"] == 1 and "cpu_baseline" not in line
    prod = np.load(tmp_path / "msm" / "double_mul.npy")
    assert prod.shape == (2048, 32) and np.load(tmp_path / "msm" / "double_mul_ok.npy").min() == 1
    g = torch.Generator(device="cpu").manual_seed(seed)

    def scalars(count):                  # bench.py's measure_msm draws its operands from one seeded generator, in this order
        t = torch.randint(0, 256, (count, 32), dtype=torch.uint8, generator=g)
        t[:, 31] &= 0x0F
        return t.numpy().tobytes()

    k, r, x = scalars(2048), scalars(2048), scalars(2048)          # [k]P + [r]G with P = [x]G
    bk, bx = scalars(1 << 16), scalars(1 << 16)                    # one 65 536-term product over points [x]G
    for i in range(2048):
        p = oracle.point_mul_generator(x[32 * i : 32 * i + 32])
        assert bytes(prod[i].astype(np.uint8)) == oracle.point_double_mul_generator(k[32 * i : 32 * i + 32], p, r[32 * i : 32 * i + 32]), i
    bp = b"".join(oracle.point_mul_generator(bx[32 * i : 32 * i + 32]) for i in range(1 << 16))
    assert bytes(np.load(tmp_path / "msm" / "multi_mul_65536.npy").astype(np.uint8)) == oracle.point_multi_mul(bk, bp)


def test_host_buffer_path_matches_device_path(eg, ctx, pk):
    """eg_verify_choice_batch (host buffers, pipelined uploads: a small first piece, then chunk-sized ones) must give the
    verdicts and the tally of the device-pointer path on the same 300 000 ballots, 1 % of them tampered."""
    import torch

    n = 300_000
    p = eg.ChoiceParams.single_choice(ctx, pk, 5)
    sz = p.ballot_size
    d = torch.empty(n * sz, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(8086, 0, n, d.data_ptr())
    ctx.synchronize()
    bad = torch.randperm(n, generator=torch.Generator().manual_seed(5))[: n // 100].cuda()
    d.view(n, sz)[bad, sz - 32] ^= 1
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    p.tally_reset()
    p.verify_batch_device(n, d.data_ptr(), st.data_ptr())
    want_tally = p.tally_encode()
    want = st.cpu().tolist()
    got, tally = p.verify_batch(d.cpu().numpy().tobytes())
    assert got == want and tally == want_tally
    assert sum(1 for s in got if s) == n // 100


# ------------------------------------------------------------------ round 4: in-process multi-GPU entry, stream hygiene on failure
@pytest.mark.parametrize("kind", ["single", "qv"])
def test_in_process_multi_device_entry(eg, ctx, oracle, pk, kind):
    """eg_verify_*_batch_multi (SURVEY 8b `device_mask`; the host of examples/voting.rs:179-213 is ONE process): contiguous slabs over
    several params objects, each on its own context, one host thread per object inside the library, tallies merged in the library.
    One GPU on the box: two and three contexts on device 0 stand in for two and three GPUs.  Verdicts (1 % tampered), the batch
    tally and the sum of the running tallies must equal the single-context result and the oracle's."""
    if kind == "single":
        op = oracle.ChoiceParams(pk, 5, True)
        mk = lambda c: eg.ChoiceParams.single_choice(c, pk, 5)
        n = 3001
    else:
        op = oracle.QvParams(pk, 3, 6)
        mk = lambda c: eg.QuadraticVotingParams(c, pk, 3, 6)
        n = 1203
    ballots = bytearray(op.generate_batch(2718, 0, n, threads=8))
    sz = len(ballots) // n
    for i in range(0, n, 100):
        ballots[i * sz + sz - 40] ^= 4
    ballots = bytes(ballots)
    want = op.verify_batch(ballots, threads=8)
    want_tally = op.tally(ballots, want)
    assert 0 < want.count(0) < n
    single = mk(ctx)
    st1, t1 = single.verify_batch(ballots)
    assert st1 == want and t1 == want_tally
    extra = [eg.Context(0), eg.Context(0)]
    try:
        for n_dev in (2, 3):
            objs = [single] + [mk(c) for c in extra[: n_dev - 1]]
            for o in objs:
                o.tally_reset()
            st, t = eg.verify_batch_multi(objs, ballots)
            assert st == want
            assert t == want_tally
            assert eg.tally_encode_multi(objs) == want_tally
            # every object tallied its own slab only (distributed.shard_range's split)
            b0, e0 = 0, n // n_dev
            assert objs[0].tally_encode() == op.tally(ballots[: e0 * sz], want[:e0])
            st_again, t_none = eg.verify_batch_multi(objs, ballots, with_tally=False)       # running tallies accumulate
            assert st_again == want and t_none is None
            grp = eg.Ristretto(ctx)
            assert eg.tally_encode_multi(objs) == grp.element_add(want_tally, want_tally)[0]
            st_e, t_e = eg.verify_batch_multi(objs, b"")                                      # an empty batch
            assert st_e == [] and t_e == bytes(64 * single.n_options)
            for o in objs[1:]:
                o.close()
        with pytest.raises(eg.EgError):
            eg.verify_batch_multi([single, single], ballots)                                  # one object per slab
    finally:
        for c in extra:
            c.close()


@pytest.mark.parametrize("kind", ["single", "qv"])
def test_in_process_multi_device_entry_on_device_buffers(eg, ctx, oracle, pk, kind):
    """eg_verify_*_batch_multi_device (VERDICT r4 task 6b): every slab already resident on its GPU, one device pointer, one status
    buffer and one stream per params object, nothing copied.  Three contexts on device 0 stand in for three GPUs; slabs of unequal
    size (one of them empty), 1 % tampered.  Verdicts per slab, the call's tally, the running tallies and their sum equal the
    oracle's; a retry after a refused call (params of another election, a null pointer for a non-empty slab) finds the running tallies
    untouched; eg_*_tally_encode_multi refuses params objects of different elections."""
    import torch

    if kind == "single":
        op = oracle.ChoiceParams(pk, 5, True)
        mk = lambda c, key=pk: eg.ChoiceParams.single_choice(c, key, 5)
        counts = [1500, 0, 901]
    else:
        op = oracle.QvParams(pk, 3, 6)
        mk = lambda c, key=pk: eg.QuadraticVotingParams(c, key, 3, 6)
        counts = [700, 0, 333]
    n = sum(counts)
    ballots = bytearray(op.generate_batch(31415, 0, n, threads=8))
    sz = len(ballots) // n
    for i in range(0, n, 100):
        ballots[i * sz + sz - 40] ^= 4
    ballots = bytes(ballots)
    want = op.verify_batch(ballots, threads=8)
    want_tally = op.tally(ballots, want)
    extra = [eg.Context(0), eg.Context(0)]
    objs = [mk(ctx)] + [mk(c) for c in extra]
    try:
        offs = [0, counts[0], counts[0] + counts[1]]
        d_b = [torch.frombuffer(bytearray(ballots[o * sz : (o + c) * sz] or b"\0"), dtype=torch.uint8).cuda() for o, c in zip(offs, counts)]
        d_s = [torch.full((max(c, 1),), 99, dtype=torch.int32, device="cuda") for c in counts]
        streams = [torch.cuda.Stream() for _ in counts]
        torch.cuda.synchronize()
        for o in objs:
            o.tally_reset()
        t = eg.verify_batch_multi_device(objs, counts, [x.data_ptr() for x in d_b], [x.data_ptr() for x in d_s],
                                         [s.cuda_stream for s in streams], with_tally=True)
        got = [int(v) & 0xFFFFFFFF for x, c in zip(d_s, counts) for v in x[:c].cpu().tolist()]
        assert got == want and t == want_tally and eg.tally_encode_multi(objs) == want_tally
        for k in (0, 2):                # every object tallied its own slab only
            assert objs[k].tally_encode() == op.tally(ballots[offs[k] * sz : (offs[k] + counts[k]) * sz], want[offs[k] : offs[k] + counts[k]])
        assert objs[1].tally_encode() == bytes(64 * objs[1].n_options)
        # the null streams, no tally asked for: the running tallies accumulate
        assert eg.verify_batch_multi_device(objs, counts, [x.data_ptr() for x in d_b], [x.data_ptr() for x in d_s]) is None
        grp = eg.Ristretto(ctx)
        twice = grp.element_add(want_tally, want_tally)[0]
        assert eg.tally_encode_multi(objs) == twice
        # refused calls leave the running tallies alone
        with pytest.raises(eg.EgError, match="null device pointer"):
            eg.verify_batch_multi_device(objs, counts, [d_b[0].data_ptr(), 0, 0], [x.data_ptr() for x in d_s])
        other_key = oracle.point_mul_generator(sc(987654321))
        stranger = mk(extra[0], other_key)
        with pytest.raises(eg.EgError, match="different elections"):
            eg.verify_batch_multi_device([objs[0], stranger], counts[:2], [d_b[0].data_ptr(), 0], [d_s[0].data_ptr(), 0])
        with pytest.raises(eg.EgError, match="different elections"):
            eg.tally_encode_multi([objs[0], stranger])
        with pytest.raises(eg.EgError, match="different elections"):
            eg.verify_batch_multi([objs[0], stranger], ballots)
        stranger.close()
        assert eg.tally_encode_multi(objs) == twice
    finally:
        for o in objs:
            o.close()
        for c in extra:
            c.close()


def test_failure_between_fork_and_join_leaves_a_usable_engine():
    """an error return between the fork onto the two work sets' streams and the join must still tie the streams
    back into the caller's.  The failure is injected by a SECOND build of the library that has fault points (tests/faultlib: the
    shipped libeg_hip.so has none, VERDICT r4 task 5), loaded through EG_LIB by a child process that runs
    tests/faultlib/scenario_fork_join.py: engine_verify_device returns an error with the first chunk's kernels queued; the same params
    object must then verify a clean batch with the right verdicts and tally."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    lib = root / "tests" / "faultlib" / "libeg_hip_faults.so"
    subprocess.check_call(["make", "-C", str(lib.parent), "-j2"], stdout=subprocess.DEVNULL)     # up to date when it travelled with the snapshot
    shipped = (root / "elastic_elgamal_amd" / "libeg_hip.so").read_bytes()
    assert b"EG_TEST_FAIL" not in shipped and b"injected failure" not in shipped   # neither a switch nor the dead branch behind it
    assert b"EG_TEST_FAIL_after_fork" in lib.read_bytes()
    r = subprocess.run([sys.executable, str(lib.parent / "scenario_fork_join.py")], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, EG_LIB=str(lib)), cwd=str(root))
    assert r.returncode == 0 and "fork/join fault scenario ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_configs4_eight_shards_on_one_gpu(eg, ctx, pk):
    """BASELINE configs[4] (10 M single-choice ballots over EIGHT GPUs) with the eight ranks played one after the other by the one GPU
    of the box (eight GPU processes at once are more than the pool admits): rank r's slab [1.25 M r, 1.25 M (r + 1)) is generated,
    1 % tampered, verified and tallied from a reset tally exactly as bench.py's step does; the eight encoded tallies then go through
    eg_points_sum_device the way the all-gathered tallies do.  The merged tally must equal the running tally of one engine that
    verified all ten million (examples/voting.rs:199-203), with 9 900 000 ballots accepted."""
    import torch

    from elastic_elgamal_amd.distributed import shard_range

    world, total = 8, 10_000_000
    p = eg.ChoiceParams.single_choice(ctx, pk, 5)          # the eight "ranks"
    whole = eg.ChoiceParams.single_choice(ctx, pk, 5)      # one engine over everything, never reset
    whole.tally_reset()
    gathered = torch.empty(world, 320, dtype=torch.uint8, device="cuda")
    accepted = 0
    for r in range(world):
        lo, hi = shard_range(total, r, world)
        n = hi - lo
        assert n == 1_250_000
        d = torch.empty(n * p.ballot_size, dtype=torch.uint8, device="cuda")
        p.encrypt_batch_device(20260612, lo, n, d.data_ptr())
        ctx.synchronize()
        g = torch.Generator(device="cpu").manual_seed(20260612 + r)
        bad = torch.randperm(n, generator=g)[: n // 100].to("cuda")
        d.view(n, p.ballot_size)[bad, p.ballot_size - 32] ^= 1
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        p.tally_reset()
        p.verify_batch_device(n, d.data_ptr(), st.data_ptr())
        p.tally_encode_device(gathered[r].data_ptr())
        whole.verify_batch_device(n, d.data_ptr(), st.data_ptr())
        ctx.synchronize()
        accepted += int((st == 0).sum().item())
        del d, st
    assert accepted == 9_900_000
    out = torch.empty(320, dtype=torch.uint8, device="cuda")
    n_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.points_sum_device(world, 10, gathered.data_ptr(), out.data_ptr(), d_bad=n_bad.data_ptr())
    ctx.synchronize()
    assert int(n_bad.item()) == 0
    assert bytes(out.cpu().numpy()) == whole.tally_encode()


@pytest.mark.parametrize("single,n_opt,groups", [(True, 5, ("0", "1", "2", "3", "4")), (False, 16, ("0", "3", "4", "8")), (True, 9, ("0", "4", "8"))])
def test_ring_group_walk_gives_the_same_verdicts(eg, ctx, oracle, pk, monkeypatch, single, n_opt, groups):
    """The ring-group walk (the comb tables of one group of rings at a time, the sums of bases accumulated group by
    group) is a schedule, not a different computation: for every group size - EG_RING_GROUP = rings per group, 0 = every table of a
    ballot at once - verdicts and tally equal the oracle's on a batch with tampered ring responses in different groups, tampered
    sum proofs, a bad point and a bad scalar (choice.rs:358-380 order of checks)."""
    op = oracle.ChoiceParams(pk, n_opt, single)
    n = 700
    ballots = bytearray(op.generate_batch(777, 0, n, n_selected=0 if single else 3, threads=8))
    sz = len(ballots) // n
    ring0 = 64 * n_opt                                     # e0, then 2 responses per ring
    for i in range(0, n, 9):                               # a response of ring (i mod n_opt): every group gets its share
        ballots[i * sz + ring0 + 32 * (1 + 2 * (i % n_opt) + (i // 9) % 2) + 5] ^= 0x10
    if single:
        for i in range(4, n, 31):                          # the sum proof (verified after the last group)
            ballots[i * sz + sz - 20] ^= 2
    ballots[13 * sz + 64 * (n_opt - 1) + 3] ^= 0x80        # a point of the last ring
    ballots[14 * sz + ring0 + 31] |= 0xf0                  # e0 not canonical
    ballots = bytes(ballots)
    want = op.verify_batch(ballots, threads=8)
    want_tally = op.tally(ballots, want)
    assert len(set(want)) >= (4 if single else 3)
    for g in groups:
        monkeypatch.setenv("EG_RING_GROUP", g)
        desc = eg.plan_describe("single" if single else "multi", n_opt)
        assert desc["ring_group"] == (int(g) if int(g) < n_opt else 0)
        p = eg.ChoiceParams(ctx, pk, n_opt, single)
        st, tally = p.verify_batch(ballots)
        assert st == want, g
        assert tally == want_tally, g
        p.close()


def test_bucket_method_multi_scalar_mul(eg, ctx, grp, oracle, monkeypatch):
    """The bucket (Pippenger) path of Group::vartime_multi_mul (pippenger.cuh; ristretto.rs:139-145 -> dalek's Pippenger above 190 terms),
    forced at small sizes (EG_MSM_BUCKET_MIN) so that the oracle can follow: identity points, zero / edge / non-canonical-width
    scalars, ONE point repeated thousands of times (a bucket as long as the problem), a point and its negative, duplicates, two
    problems in one call, a generator term through the device entry point, an undecodable point (flagged, contributes nothing)."""
    import torch

    rnd = random.Random(2026)
    pool = [oracle.point_mul_generator(sc(rnd.randrange(L))) for _ in range(300)] + [b"\0" * 32]
    neg = [oracle.point_add(b"\0" * 32, b"\0" * 32)]          # identity again
    edge = [0, 1, 2, L - 1, L - 2, 2**252, 2**252 - 1, (1 << 15) - 1, 1 << 15, 1 << 14, (1 << 14) + 1, 8, 0x0888888888888888888888888888888888888888888888888888888888888888]
    monkeypatch.setenv("EG_MSM_BUCKET_MIN", "4096")      # read once, by eg_init: a context of its own for each setting
    default_ctx, default_grp = ctx, grp
    ctx = eg.Context(0)
    grp = eg.Ristretto(ctx)
    for terms, m, mode in ((4096, 1, "random"), (5003, 2, "random"), (4096, 1, "one_point"), (6001, 1, "edge"), (20001, 1, "random")):
        if mode == "one_point":
            scal = [[sc(rnd.randrange(1, 9)) for _ in range(terms)] for _ in range(m)]       # digits 1..8 of window 0 only: eight huge buckets
            pp = [[pool[3]] * terms for _ in range(m)]
        elif mode == "edge":
            scal = [[sc(edge[t % len(edge)]) for t in range(terms)] for _ in range(m)]
            pp = [[pool[t % 7] if t % 3 else pool[-1] for t in range(terms)] for _ in range(m)]
        else:
            scal = [[sc(rnd.randrange(L)) for _ in range(terms)] for _ in range(m)]
            pp = [[pool[rnd.randrange(len(pool))] for _ in range(terms)] for _ in range(m)]
        sb, pb = b"".join(b"".join(x) for x in scal), b"".join(b"".join(x) for x in pp)
        got, ok = grp.vartime_multi_mul(terms, sb, pb)
        assert set(ok) == {1}, (terms, mode)
        for i in range(m):
            assert got[32 * i : 32 * i + 32] == oracle.point_multi_mul(b"".join(scal[i]), b"".join(pp[i])), (terms, mode, i)
        r = b"".join(sc(rnd.randrange(L)) for _ in range(m))
        ds = torch.frombuffer(bytearray(sb), dtype=torch.uint8).cuda()
        dp = torch.frombuffer(bytearray(pb), dtype=torch.uint8).cuda()
        dr = torch.frombuffer(bytearray(r), dtype=torch.uint8).cuda()
        do = torch.zeros(32 * m, dtype=torch.uint8, device="cuda")
        dok = torch.zeros(m, dtype=torch.uint8, device="cuda")
        need = grp.msm_scratch_bytes(m, terms)
        assert need > 0
        scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")
        grp.vartime_multi_mul_device(m, terms, ds.data_ptr(), dp.data_ptr(), do.data_ptr(), d_r=dr.data_ptr(), d_scratch=scratch.data_ptr(), d_ok=dok.data_ptr())
        ctx.synchronize()
        out = bytes(do.cpu().numpy())
        for i in range(m):
            assert out[32 * i : 32 * i + 32] == oracle.point_add(got[32 * i : 32 * i + 32], oracle.point_mul_generator(r[32 * i : 32 * i + 32])), (terms, mode, i)
        assert dok.cpu().tolist() == [1] * m
        _check_prepared_points(eg, ctx, grp, m, terms, ds, dp, dr, out)
        with pytest.raises(eg.EgError):          # the bucket path cannot run without its scratch
            grp.vartime_multi_mul_device(m, terms, ds.data_ptr(), dp.data_ptr(), do.data_ptr())
        if mode == "random" and m == 2:          # an undecodable point in problem 1: flagged, and it contributes the identity
            bad = bytearray(pb)
            bad[(terms + 77) * 32 : (terms + 78) * 32] = b"\xff" * 32
            out2, ok2 = grp.vartime_multi_mul(terms, sb, bytes(bad))
            assert list(ok2) == [1, 0] and out2[:32] == got[:32]
            rest_s = b"".join(scal[1][:77] + scal[1][78:]); rest_p = b"".join(pp[1][:77] + pp[1][78:])
            assert out2[32:] == oracle.point_multi_mul(rest_s, rest_p)
            # prepared: the prepare call flags it and prepares the identity, so the product is the one without that term
            dbad = torch.frombuffer(bytearray(bad), dtype=torch.uint8).cuda()
            prep = torch.zeros(m * terms * 96, dtype=torch.uint8, device="cuda")
            pok = torch.zeros(m * terms, dtype=torch.uint8, device="cuda")
            grp.prepare_points_device(m * terms, dbad.data_ptr(), prep.data_ptr(), d_ok=pok.data_ptr())
            grp.vartime_multi_mul_prepared_device(m, terms, ds.data_ptr(), prep.data_ptr(), do.data_ptr(), d_scratch=scratch.data_ptr())
            ctx.synchronize()
            flags = pok.cpu().tolist()
            assert flags.count(0) == 1 and flags[terms + 77] == 0
            assert bytes(do.cpu().numpy()) == out2
    # a size of the order of the default switch (2^20 terms): both paths must give the same encoding on the same operands
    terms = (1 << 17) + 12345
    g = torch.Generator(device="cpu").manual_seed(5)
    s_t = torch.randint(0, 256, (terms, 32), dtype=torch.uint8, generator=g)
    s_t[:, 31] &= 0x0F
    base = torch.frombuffer(bytearray(b"".join(pool[:256])), dtype=torch.uint8)
    p_t = base.view(256, 32)[torch.randint(0, 256, (terms,), generator=g)].contiguous()
    ds, dp = s_t.reshape(-1).cuda(), p_t.reshape(-1).cuda()
    outs, sizes = [], []
    monkeypatch.setenv("EG_MSM_BUCKET_MIN", str(1 << 30))
    straus_ctx = eg.Context(0)
    monkeypatch.delenv("EG_MSM_BUCKET_MIN")
    for c in (ctx, straus_ctx):
        g2 = eg.Ristretto(c)
        do = torch.zeros(32, dtype=torch.uint8, device="cuda")
        sizes.append(g2.msm_scratch_bytes(1, terms))
        scratch = torch.zeros(max(sizes[-1], 16), dtype=torch.uint8, device="cuda")
        g2.vartime_multi_mul_device(1, terms, ds.data_ptr(), dp.data_ptr(), do.data_ptr(), d_scratch=scratch.data_ptr())
        c.synchronize()
        outs.append(bytes(do.cpu().numpy()))
    assert outs[0] == outs[1] != bytes(32)
    assert sizes[0] != sizes[1]                  # the scratch a call needs is the CONTEXT's answer (its switch is fixed at eg_init) ...
    # ... so changing the environment afterwards changes nothing for a live context (a buffer sized for one path, a launch on the other)
    monkeypatch.setenv("EG_MSM_BUCKET_MIN", str(1 << 30))
    assert eg.Ristretto(ctx).msm_scratch_bytes(1, terms) == sizes[0]
    monkeypatch.delenv("EG_MSM_BUCKET_MIN")
    straus_ctx.close()
    ctx.close()
    grp = default_grp
    assert grp.msm_scratch_bytes(1, 1 << 20) > 100 << 20       # by default the bucket path takes over at 2^20 terms (and needs its scratch) ...
    assert grp.msm_scratch_bytes(1, (1 << 20) - 1) < 64 << 20  # ... and Straus' partial sums are all that is needed below


def test_ring_group_walk_over_many_chunks(eg, ctx, pk, monkeypatch):
    """The ring-group walk across chunk and work-set boundaries: 300 000 single-choice ballots (1 % tampered) in chunks of 65 536 on the
    two work sets, grouped (2 rings per group: the accumulators of the sum tables are re-used chunk after chunk) against the ungrouped
    engine on the same device buffer: identical verdicts and tally."""
    import torch

    n = 300_000
    monkeypatch.setenv("EG_CHUNK", "65536")
    monkeypatch.setenv("EG_RING_GROUP", "0")
    plain = eg.ChoiceParams.single_choice(ctx, pk, 5)
    monkeypatch.setenv("EG_RING_GROUP", "2")
    grouped = eg.ChoiceParams.single_choice(ctx, pk, 5)
    assert eg.plan_describe("single", 5)["table_groups"] == 3
    d = torch.empty(n * plain.ballot_size, dtype=torch.uint8, device="cuda")
    plain.encrypt_batch_device(424242, 0, n, d.data_ptr())
    ctx.synchronize()
    g = torch.Generator(device="cpu").manual_seed(7)
    bad = torch.randperm(n, generator=g)[: n // 100].to("cuda")
    d.view(n, plain.ballot_size)[bad[: n // 200], plain.ballot_size - 32] ^= 1          # sum proofs ...
    d.view(n, plain.ballot_size)[bad[n // 200 :], 64 * 5 + 32 * 4 + 7] ^= 4             # ... and a response of ring 1
    st_a = torch.empty(n, dtype=torch.int32, device="cuda")
    st_b = torch.empty(n, dtype=torch.int32, device="cuda")
    for p, st in ((plain, st_a), (grouped, st_b)):
        p.tally_reset()
        p.verify_batch_device(n, d.data_ptr(), st.data_ptr())
    ctx.synchronize()
    assert torch.equal(st_a, st_b)
    assert int((st_a == 0).sum()) == n - n // 100
    assert plain.tally_encode() == grouped.tally_encode()


# ------------------------------------------------------------------ round 6: the context's shared workspace, held multi calls, the new entries
def _gpu_ballots_as_json(eg, p, seed, distinct, reps, tamper_every=0, **gen_kw):
    """distinct GPU-generated ballots (every tamper_every-th tampered) -> (packed bytes of the distinct ones, JSON array text repeating them)."""
    import json

    import torch
    from elastic_elgamal_amd import ingest, serde

    sz = p.ballot_size
    d = torch.empty(distinct * sz, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(seed, 0, distinct, d.data_ptr(), **gen_kw)
    p.ctx.synchronize()
    raw = bytearray(d.cpu().numpy().tobytes())
    if tamper_every:
        for i in range(0, distinct, tamper_every):
            raw[i * sz + sz - 32] ^= 1
    raw = bytes(raw)
    if p.kind_name == "qv":
        one = [json.dumps(ingest.unpack_qv_ballot(raw[i * sz : (i + 1) * sz], p.n_options, p.credits)) for i in range(distinct)]
    else:
        one = [json.dumps(serde.unpack_encrypted_choice(raw[i * sz : (i + 1) * sz], p.n_options, p.single)) for i in range(distinct)]
    return raw, ("[" + ",".join(one * reps) + "]").encode()


def test_two_params_objects_of_one_context_work_at_the_same_time(eg, ctx, grp, oracle, pk):
    """the per-lane workspace belongs to the CONTEXT; a JSON stream's submissions are in flight while the context's lock
    is free, so a second params object of the same context - or the primitive tier - can enqueue kernels that use the same workspace on
    other streams.  The library orders every user of the workspace behind the previous one with events (ws_acquire / ws_release).
    (a) two params objects (single-choice and quadratic voting) run eg_verify_*_json on ~10^5 ballots each from two threads while a
    third thread multiplies through the primitive tier; (b) with a stream open and half fed, the SAME thread calls the primitive tier and
    verifies on another object.  Everything against the oracle."""
    import threading

    p1 = eg.ChoiceParams.single_choice(ctx, pk, 5)
    p2 = eg.QuadraticVotingParams(ctx, pk, 3, 9)
    o1, o2 = oracle.ChoiceParams(pk, 5, True), oracle.QvParams(pk, 3, 9)
    raw1, text1 = _gpu_ballots_as_json(eg, p1, 9001, 400, 300, tamper_every=7)
    raw2, text2 = _gpu_ballots_as_json(eg, p2, 9002, 200, 250, tamper_every=5)
    want1, want2 = o1.verify_batch(raw1, threads=8), o2.verify_batch(raw2, threads=8)
    assert 0 < want1.count(0) < 400 and 0 < want2.count(0) < 200
    rnd = random.Random(6)
    ks = b"".join(sc(rnd.randrange(L)) for _ in range(3 * 96))
    pts = b"".join(oracle.point_mul_generator(sc(rnd.randrange(L))) for _ in range(3 * 96))
    want_msm = b"".join(oracle.point_multi_mul(ks[96 * i : 96 * i + 96], pts[96 * i : 96 * i + 96]) for i in range(96))
    errors, running = [], [True]

    def json_worker(p, text, want, reps):
        try:
            for _ in range(3):
                got, _ = p.verify_json(text, max_objects=len(want) * reps, threads=4)
                assert got == want * reps, [(i, a, b) for i, (a, b) in enumerate(zip(got, want * reps)) if a != b][:4]
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def msm_worker():
        try:
            while running[0]:
                out, ok = grp.vartime_multi_mul(3, ks, pts)
                assert out == want_msm and set(ok) == {1}
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=json_worker, args=(p1, text1, want1, 300)), threading.Thread(target=json_worker, args=(p2, text2, want2, 250))]
    third = threading.Thread(target=msm_worker)
    for t in threads + [third]:
        t.start()
    for t in threads:
        t.join()
    running[0] = False
    third.join()
    assert not errors, errors
    # (b) one thread: a stream half fed (its submissions in flight), then the primitive tier and another object, then the rest
    st = p1.json_stream(threads=4)
    half = len(text1) // 2
    st.feed(text1[:half])
    for _ in range(3):
        out, ok = grp.vartime_multi_mul(3, ks, pts)
        assert out == want_msm and set(ok) == {1}
        assert p2.verify_batch(raw2)[0] == want2
    st.feed(text1[half:])
    got, _ = st.end()
    assert got == want1 * 300
    p1.close(); p2.close()


def test_multi_calls_hold_their_params_objects(eg, ctx, grp, oracle, pk):
    """(a) a multi-GPU call on a params object that an explicitly opened JSON stream owns is refused BEFORE it touches
    anything - the stream's share of the tally and the running tally it set aside are intact: the stream ends with the verdicts and the
    tally of the one-shot entry; (b) while a multi call runs, calls of other threads on its objects wait (they used to interleave with
    the set-aside / roll-back of the running tallies): after three threads have hammered two objects with multi calls, host calls and
    one-shot JSON calls, every running tally is exactly the sum of the calls made."""
    import threading

    c2 = eg.Context(0)
    a, b = eg.ChoiceParams.single_choice(ctx, pk, 5), eg.ChoiceParams.single_choice(c2, pk, 5)
    op = oracle.ChoiceParams(pk, 5, True)
    raw, text = _gpu_ballots_as_json(eg, a, 9003, 300, 40, tamper_every=9)
    sz = a.ballot_size
    want = op.verify_batch(raw, threads=8)
    T = op.tally(raw, want)                       # tally of the 300 distinct ballots
    zero = bytes(64 * 5)

    def times(t, k):                              # k x an encoded tally, through the primitive tier
        acc = zero
        for _ in range(k):
            acc = grp.element_add(acc, t)[0]
        return acc

    want_json, want_json_tally = b.verify_json(text, max_objects=300 * 40)
    assert want_json == want * 40 and want_json_tally == times(T, 40)
    a.tally_reset(); b.tally_reset()
    # (a) refused while a stream is open on one of the objects, with everything intact
    st = b.json_stream(threads=4)
    st.feed(text[: len(text) // 2])
    with pytest.raises(eg.EgError, match="JSON stream is open"):
        eg.verify_batch_multi([a, b], raw)
    with pytest.raises(eg.EgError, match="JSON stream is open"):
        eg.tally_encode_multi([a, b])
    st.feed(text[len(text) // 2 :])
    got, tally = st.end()
    assert got == want_json and tally == want_json_tally == b.tally_encode() and a.tally_encode() == zero
    a.tally_reset(); b.tally_reset()
    # (b) three threads on the same two objects
    errors = []
    half = (300 // 2) * sz

    def multi_worker():
        try:
            for _ in range(4):
                stt, t = eg.verify_batch_multi([a, b], raw)
                assert stt == want and t == T
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def host_worker():
        try:
            for _ in range(6):
                assert a.verify_batch(raw[:half])[0] == want[:150]
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def json_worker():
        try:
            for _ in range(2):
                got, t = b.verify_json(text, max_objects=300 * 40, threads=4)
                assert got == want_json and t == want_json_tally
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=f) for f in (multi_worker, host_worker, json_worker)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    Ta, Tb = op.tally(raw[:half], want[:150]), op.tally(raw[half:], want[150:])           # the slabs of a multi call over two objects
    want_a = grp.element_add(times(Ta, 4), times(Ta, 6))[0]                                 # 4 multi slabs + 6 host calls on the first half
    want_b = grp.element_add(times(Tb, 4), times(want_json_tally, 2))[0]                    # 4 multi slabs + 2 JSON texts
    assert a.tally_encode() == want_a and b.tally_encode() == want_b
    assert eg.tally_encode_multi([a, b]) == grp.element_add(want_a, want_b)[0]
    a.close(); b.close(); c2.close()


def test_selfbench_abi_version_and_prepared_point_arguments(eg, ctx, grp):
    """eg_selfbench_fmul (VERDICT r5 task 6): the shipped fe_mul in a bare chain sustains 200-320 G multiplications/s on an MI355X at
    2.0-2.5 GHz; eg_abi_version is what the header says; eg_points_prepare_device insists on d_ok and on a 16-byte aligned d_prepared
    (ADVICE r5, low)."""
    import re
    from pathlib import Path

    import torch

    g, mhz = ctx.selfbench_fmul(1.0)
    assert 200 < g < 320 and 1800 < mhz < 2600, (g, mhz)
    hdr = (Path(__file__).resolve().parent.parent / "include" / "eg_hip.h").read_text()
    assert eg._load().eg_abi_version() == int(re.search(r"#define EG_ABI_VERSION (\d+)", hdr).group(1)) == eg.ABI_VERSION
    enc = torch.zeros(32 * 8, dtype=torch.uint8, device="cuda")
    prep = torch.zeros(eg.prepared_point_size() * 8 + 16, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(8, dtype=torch.uint8, device="cuda")
    with pytest.raises(eg.EgError, match="d_ok is mandatory"):
        grp.prepare_points_device(8, enc.data_ptr(), prep.data_ptr(), 0)
    with pytest.raises(eg.EgError, match="16-byte aligned"):
        grp.prepare_points_device(8, enc.data_ptr(), prep.data_ptr() + 4, ok.data_ptr())
    grp.prepare_points_device(8, enc.data_ptr(), prep.data_ptr(), ok.data_ptr())
    ctx.synchronize()
    assert ok.cpu().tolist() == [1] * 8                     # the all-zero encoding is the identity, a valid element


def test_json_feed_owned_and_the_bound_on_wrong_shape_text(eg, ctx, oracle, pk, monkeypatch):
    """eg_verify_json_feed_owned (VERDICT r5 task 4b): blocks handed over without a copy - the release function is called once per block,
    by end at the latest - give the verdicts and the tally of the one-shot entry; an aborted stream gives every block back too.  A text
    made of ballots of another shape than the election's stops at EG_JSON_ODD_MAX_MB instead of buffering its input;
    a one-shot call whose text holds more objects than max_objects breaks off while parsing."""
    import ctypes as C
    import json

    import elastic_elgamal_amd as egmod

    p = eg.ChoiceParams.single_choice(ctx, pk, 5)
    op = oracle.ChoiceParams(pk, 5, True)
    raw, text = _gpu_ballots_as_json(eg, p, 9004, 200, 100, tamper_every=11)
    want = op.verify_batch(raw, threads=8) * 100
    one_shot, one_tally = p.verify_json(text, max_objects=len(want))
    assert one_shot == want
    base = C.cast(C.c_char_p(text), C.c_void_p).value
    for piece in (1 << 20, 12_345, 1 << 26):
        before = egmod.released_blocks()
        st = p.json_stream(threads=4)
        n_blocks = 0
        for at in range(0, len(text), piece):
            st.feed_owned_ptr(base + at, min(piece, len(text) - at))
            n_blocks += 1
        got, tally = st.end()
        assert got == want and tally == one_tally
        assert egmod.released_blocks() - before == n_blocks
    before = egmod.released_blocks()
    st = p.json_stream(threads=2)
    for at in range(0, len(text), 1 << 16):
        st.feed_owned_ptr(base + at, min(1 << 16, len(text) - at))
    st.abort()
    assert egmod.released_blocks() - before == -(-len(text) // (1 << 16))
    assert p.verify_json(text, max_objects=len(want)) == (one_shot, one_tally)
    with pytest.raises(eg.EgError, match="max_objects"):
        p.verify_json(text, max_objects=len(want) // 3)
    assert p.verify_json(text, max_objects=len(want)) == (one_shot, one_tally)
    p.close()
    # ballots of a 4-option election offered to a 5-option one: each deserialises, none has the election's shape
    monkeypatch.setenv("EG_JSON_ODD_MAX_MB", "1")
    q = eg.ChoiceParams.single_choice(ctx, pk, 5)
    monkeypatch.delenv("EG_JSON_ODD_MAX_MB")
    p4 = eg.ChoiceParams.single_choice(ctx, pk, 4)
    _, odd = _gpu_ballots_as_json(eg, p4, 9005, 50, 40)            # 2000 objects, ~2.5 MB of text
    with pytest.raises(eg.EgError, match="EG_JSON_ODD_MAX_MB"):
        q.verify_json(odd, max_objects=2000)
    small = json.dumps(json.loads(odd)[:50]).encode()
    got, _ = q.verify_json(small, max_objects=50)                   # below the bound the object path resolves them: OptionsLenMismatch
    assert got == [eg.OPTIONS_LEN] * 50
    p4.close(); q.close()


@pytest.mark.parametrize("kind", ["single", "qv"])
def test_json_entries_over_several_params_objects(eg, ctx, grp, oracle, pk, kind, monkeypatch):
    """eg_verify_*_json_multi / eg_verify_*_json_begin_multi (VERDICT r5 task 4a; examples/voting.rs:195-198 is the producer, src/serde.rs:19-80
    the layout): ONE parser, its packed windows dealt to three params objects (three contexts on device 0 stand in for three GPUs), verdicts in
    TEXT order.  Verdicts and tally equal the one-object entry's on the same text - tampered ballots, a junk object, ballots of another
    shape (resolved through the first object); every lane took part; the running tallies add up to the text's tally; the stream form fed in
    random pieces, with take() handing out only final verdicts, gives the same; a params object of the stream refuses other calls; abort
    leaves every running tally as it was."""
    import json

    rnd = random.Random(77)
    monkeypatch.setenv("EG_JSON_WINDOW_KB", "96")         # many windows in a small text: every lane gets some
    monkeypatch.setenv("EG_JSON_FIRST_MIN", "64")
    extra = [eg.Context(0), eg.Context(0)]
    if kind == "single":
        mk = lambda c, n=5: eg.ChoiceParams.single_choice(c, pk, n)
        op = oracle.ChoiceParams(pk, 5, True)
    else:
        mk = lambda c, n=3: eg.QuadraticVotingParams(c, pk, n, 9)
        op = oracle.QvParams(pk, 3, 9)
    objs = [mk(ctx)] + [mk(c) for c in extra]
    other = mk(ctx, 4)                                       # an election of another shape: its ballots deserialise, but not as ours
    monkeypatch.delenv("EG_JSON_WINDOW_KB"); monkeypatch.delenv("EG_JSON_FIRST_MIN")
    try:
        raw, text = _gpu_ballots_as_json(eg, objs[0], 9100, 300, 1, tamper_every=13)
        _, odd = _gpu_ballots_as_json(eg, other, 9101, 6, 1)
        want300 = op.verify_batch(raw, threads=8)
        items = json.loads(text) * 12
        odd_items = json.loads(odd)
        for k, o in enumerate(odd_items):
            items.insert(500 * (k + 1), o)
        items.insert(1234, {"junk": ["}", "]"]})
        whole = json.dumps(items).encode()
        one = mk(eg.Context(0))
        want, want_tally = one.verify_json(whole, max_objects=len(items))
        one.close()
        assert len(want) == len(items) and want.count(eg.MALFORMED) == 1 and want.count(0) == 12 * want300.count(0)
        assert sum(1 for v in want if eg.status_kind(v) in (eg.OPTIONS_LEN, eg.QV_VARIANT_LEN, eg.RANGE_LEN, eg.QV_CREDIT_RANGE_LEN, eg.QV_CREDIT_EQUIV_LEN)) == 6
        for o in objs:
            o.tally_reset()
        got, tally = eg.verify_json_multi(objs, whole, max_objects=len(items), threads=4)
        assert got == want and tally == want_tally
        shares = [o.tally_encode() for o in objs]
        assert all(s != bytes(len(s)) for s in shares), "a lane got no window"
        assert eg.tally_encode_multi(objs) == want_tally
        # the stream form, random pieces
        for o in objs:
            o.tally_reset()
        st = eg.json_stream_multi(objs, threads=4)
        for o in objs:
            with pytest.raises(eg.EgError, match="stream is open"):
                o.verify_batch(raw[: o.ballot_size])
        with pytest.raises(eg.EgError, match="JSON stream is open"):
            eg.verify_batch_multi(objs, raw)
        got, at = [], 0
        while at < len(whole):
            size = min(rnd.choice((1, 50, 3000, 70000, 400000)), len(whole) - at)
            st.feed(whole[at : at + size])
            at += size
            got += st.take(2000)
            assert got == want[: len(got)]
        rest, tally = st.end()
        assert got + rest == want and tally == want_tally and eg.tally_encode_multi(objs) == want_tally
        # abort: nothing moves
        before = [o.tally_encode() for o in objs]
        st = eg.json_stream_multi(objs, threads=2)
        st.feed(whole[: len(whole) // 2])
        st.abort()
        assert [o.tally_encode() for o in objs] == before
        # a text with more objects than room: breaks off, and the objects are in order afterwards
        with pytest.raises(eg.EgError, match="max_objects"):
            eg.verify_json_multi(objs, whole, max_objects=len(items) // 2)
        assert [o.tally_encode() for o in objs] == before
        got, tally = eg.verify_json_multi(objs[:2], whole, max_objects=len(items))       # two objects, one of them the first again
        assert got == want and tally == want_tally
    finally:
        for o in objs:
            o.close()
        other.close()
        for c in extra:
            c.close()
