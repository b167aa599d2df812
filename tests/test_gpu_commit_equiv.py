"""Commitment-equivalence proofs (src/proofs/commitment.rs) on the GPU: the batch verifier through eg_verify_proof_batch with the
engine's third fixed base H, and the prover kernel, against the reference's snapshot and against the test-side restatement
(tests/commit_equiv_ref.py) on EVERY item of every batch.  Bit-exact: integer and byte work."""
import ctypes as C
import random

import pytest

import commit_equiv_ref as R

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493
BAD_SCALAR_BYTES = b"\xff" * 32            # >= l
BAD_POINT_BYTES = b"\x01" + bytes(31)      # an odd ("negative") field element never is a ristretto255 encoding


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
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def key(oracle, fx):
    return oracle.keypair_from_seed(fx["seed"])[1]


@pytest.fixture(scope="module")
def h(fx):
    return bytes(fx["blinding_base"])


@pytest.fixture(scope="module")
def ver(eg, ctx, key, h):
    v = eg.CommitmentEquivalenceVerifier(ctx, key, h, b"test")
    yield v
    v.close()


@pytest.fixture(scope="module")
def snap_item(eg, fx):
    from elastic_elgamal_amd import serde

    return serde.pack_commitment_equivalence(fx["object"])


def items_of(packed):
    return [packed[k : k + R.ITEM] for k in range(0, len(packed), R.ITEM)]


def flip(item, bit):
    t = bytearray(item)
    t[bit // 8] ^= 1 << (bit % 8)
    return bytes(t)


# ------------------------------------------------------------------ snapshot
def test_snapshot_verifies_and_the_prover_reproduces_it(oracle, ver, fx, key, h, snap_item):
    assert ver.item_size == 224
    assert ver.verify(snap_item) == [0]
    got, blind = ver.prove(fx["seed"], 0, [fx["value"]], rng_skip=fx["rng_skip"], with_blindings=True)
    for i in range(R.N_ITEMS):
        assert got[32 * i : 32 * i + 32] == snap_item[32 * i : 32 * i + 32], f"item {i}"
    _, _, rng = oracle.keypair_from_seed(fx["seed"])
    want, r_c = R.prove(key, h, b"test", fx["value"], rng)
    assert want == snap_item and blind == r_c
    assert ver.prove(fx["seed"], 0, [fx["value"]], rng_skip=fx["rng_skip"]) == snap_item        # without the blinding output


# ------------------------------------------------------------------ batch
def test_batch_of_generated_and_tampered_items_matches_the_restatement_everywhere(oracle, ver, key, h):
    """100 000 items with random 64-bit values (0, 1 and 2^64 - 1 among them), a tenth of them with 1-3 flipped bits anywhere; the first
    seven tampered items carry ONE flip at a fixed place in item position 0..6.  The restatement runs over every item, on up to 16
    processes (0.7 ms per item on one core: 70 s of CPU for the batch, inside the two minutes the batch size was chosen for)."""
    n = 100_000
    rnd = random.Random(20260)
    values = [0, 1, 2**64 - 1] + [rnd.getrandbits(64) for _ in range(n - 3)]
    rnd.shuffle(values)
    packed = ver.prove(4711, 0, values)
    assert len(packed) == n * R.ITEM
    its = items_of(packed)
    # the prover against the restatement on a sample that includes the three special values (the verifier sees every item below)
    special = [values.index(0), values.index(1), values.index(2**64 - 1)] + list(range(40))
    for i in special:
        rng = oracle.rng_from_u64(4711 + i)
        assert R.prove(key, h, b"test", values[i], rng)[0] == its[i], i
    tampered = rnd.sample(range(n), n // 10)
    for k, i in enumerate(tampered):
        if k < R.N_ITEMS:
            its[i] = flip(its[i], 256 * k + 9)                    # item position k, by construction
        else:
            for _ in range(rnd.randint(1, 3)):
                its[i] = flip(its[i], rnd.randrange(8 * R.ITEM))
    packed = b"".join(its)
    got = ver.verify(packed)
    want = R.verify_parallel(key, h, b"test", packed)
    assert len(got) == len(want) == n
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (len(bad), [(i, got[i], want[i]) for i in bad[:10]])
    hit = set(tampered)
    assert all(got[i] == 0 for i in range(n) if i not in hit)
    assert all(got[i] != 0 for i in tampered[: R.N_ITEMS])
    kinds = {s & 0xFF for s in got}
    assert kinds == {R.OK, R.BAD_SCALAR, R.BAD_POINT, R.CHALLENGE}, kinds
    # malformed verdicts name every item position
    assert {s >> 8 for s in got if s & 0xFF == R.BAD_POINT} == {0, 1, 2}
    assert {s >> 8 for s in got if s & 0xFF == R.BAD_SCALAR} == {3, 4, 5, 6}


# ------------------------------------------------------------------ negatives
def test_negative_cases(eg, ctx, oracle, ver, key, h, snap_item):
    item = snap_item
    # the reference's three (commitment.rs:298-330): another ciphertext, C + G, another label
    rng = oracle.rng_from_u64(99)
    r = oracle.sc_from_wide(oracle.rng_fill64(rng))
    other_ct = oracle.point_mul_generator(r) + oracle.point_add(oracle.point_mul_generator(R.sc(8)), oracle.point_multi_mul(r, key))
    c_plus_g = oracle.point_add(item[64:96], oracle.point_mul_generator(R.ONE))
    cases = other_ct + item[64:] + item[:64] + c_plus_g + item[96:] + item
    assert ver.verify(cases) == [R.CHALLENGE, R.CHALLENGE, R.OK] == R.verify_many(key, h, b"test", cases)
    five_g = oracle.point_mul_generator(R.sc(5))
    for pk2, h2, label in ((key, h, b"other_test"), (key, five_g, b"test"), (key, key, b"test"), (five_g, h, b"test"), (h, h, b"test"),
                           (key, h, b""), (key, h, b"t" * 255)):
        v = eg.CommitmentEquivalenceVerifier(ctx, pk2, h2, label)
        try:
            assert v.verify(item) == [R.CHALLENGE] == [R.verify(pk2, h2, label, item)], (pk2 == key, h2 == h, label)
            # ... and each of them accepts what its own prover makes
            mine = v.prove(5, 0, [42, 0])
            assert v.verify(mine) == [0, 0] == R.verify_many(pk2, h2, label, mine)
            assert ver.verify(mine) == [R.CHALLENGE] * 2
        finally:
            v.close()


def test_identity_commitment_with_a_matching_proof_is_accepted(oracle, ver, key, h):
    rng = oracle.rng_from_u64(31)
    item, r_c = R.prove(key, h, b"test", 0, rng, pins={"r_c": 0})
    assert item[64:96] == bytes(32) and r_c == bytes(32)
    assert R.verify(key, h, b"test", item) == R.OK
    assert ver.verify(item) == [R.OK]
    # value 0 through the GPU prover: C = [r_c]H, accepted too; the identity C with the wrong proof is a mismatch
    mine = ver.prove(31, 0, [0])
    assert ver.verify(mine) == [R.OK]
    swapped = mine[:64] + bytes(32) + mine[96:]
    assert ver.verify(swapped) == [R.CHALLENGE] == [R.verify(key, h, b"test", swapped)]
    # all-identity elements and zero scalars: well-formed, and no proof
    assert ver.verify(bytes(R.ITEM)) == [R.verify(key, h, b"test", bytes(R.ITEM))]


def test_malformed_items_at_every_position(ver, key, h, snap_item):
    l_bytes = L.to_bytes(32, "little")
    cases = []
    for i in range(R.N_ITEMS):
        bads = [BAD_POINT_BYTES, b"\xff" * 32, (2**255 - 19).to_bytes(32, "little")] if i < R.N_POINTS else [BAD_SCALAR_BYTES, l_bytes,
                                                                                                       (L + 1).to_bytes(32, "little")]
        for b in bads:
            cases.append((snap_item[: 32 * i] + b + snap_item[32 * i + 32 :], (R.BAD_POINT if i < R.N_POINTS else R.BAD_SCALAR) | (i << 8)))
    # several malformed items: the first in wire order wins, whatever its kind
    for i in range(R.N_ITEMS):
        for j in range(i + 1, R.N_ITEMS):
            t = bytearray(snap_item)
            for k in (i, j):
                t[32 * k : 32 * k + 32] = BAD_POINT_BYTES if k < R.N_POINTS else BAD_SCALAR_BYTES
            cases.append((bytes(t), (R.BAD_POINT if i < R.N_POINTS else R.BAD_SCALAR) | (i << 8)))
    # the largest canonical scalar is well-formed (and proves nothing)
    cases.append((snap_item[:192] + (L - 1).to_bytes(32, "little"), R.CHALLENGE))
    packed = b"".join(c for c, _ in cases)
    got = ver.verify(packed)
    assert got == [w for _, w in cases]
    assert got == R.verify_many(key, h, b"test", packed)


# ------------------------------------------------------------------ lanes
def test_tampered_items_at_wavefront_and_block_edges(ver, key, h):
    n = 64 * 9 + 37           # two blocks of 256 and a ragged tail
    its = items_of(ver.prove(9, 0, list(range(n))))
    marked = [0, 63, 64, n - 1] + list(range(256, 320))            # lanes 0 / 63 / 64 / last, and a whole wavefront
    for k, i in enumerate(marked):
        its[i] = flip(its[i], (k * 53) % (8 * R.ITEM))
    packed = b"".join(its)
    got = ver.verify(packed)
    assert got == R.verify_many(key, h, b"test", packed)
    assert [i for i, s in enumerate(got) if s != 0] == sorted(marked)
    # one item, and none
    assert ver.verify(its[1]) == [0] and ver.verify(its[0]) != [0] and ver.verify(b"") == []


# ------------------------------------------------------------------ entries and tables
def test_host_and_device_entries_agree(ver, key, h):
    import torch

    n = 3000
    rnd = random.Random(5)
    vals = [rnd.getrandbits(64) for _ in range(n)]
    d_vals = torch.tensor([v - 2**64 if v >= 2**63 else v for v in vals], dtype=torch.int64, device="cuda")
    d_items = torch.zeros(n * R.ITEM, dtype=torch.uint8, device="cuda")
    d_blind = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    ver.prove_device(123, 10, n, d_vals.data_ptr(), d_items.data_ptr(), d_blind.data_ptr(), rng_skip=2)
    ver.ctx.synchronize()
    host_items, host_blind = ver.prove(123, 10, vals, rng_skip=2, with_blindings=True)
    assert bytes(d_items.cpu().numpy().tobytes()) == host_items
    assert bytes(d_blind.cpu().numpy().tobytes()) == host_blind
    # without the blinding output, on a stream of the caller's
    s = torch.cuda.Stream()
    d_items2 = torch.zeros_like(d_items)
    ver.prove_device(123, 10, n, d_vals.data_ptr(), d_items2.data_ptr(), 0, rng_skip=2, stream=s.cuda_stream)
    s.synchronize()
    assert torch.equal(d_items, d_items2)
    its = items_of(host_items)
    for i in range(0, n, 7):
        its[i] = flip(its[i], (i * 131) % (8 * R.ITEM))
    packed = b"".join(its)
    d_items.copy_(torch.frombuffer(bytearray(packed), dtype=torch.uint8))
    ver.verify_device(n, d_items.data_ptr(), d_status.data_ptr(), s.cuda_stream)
    s.synchronize()
    ver.ctx.synchronize()
    dev = [x & 0xFFFFFFFF for x in d_status.cpu().tolist()]
    assert dev == ver.verify(packed) == R.verify_many(key, h, b"test", packed)
    assert 0 < dev.count(0) < n


@pytest.mark.parametrize("big_bits", [24, 22, 0])
def test_wide_comb_tables_give_the_same_verdicts(eg, key, h, monkeypatch, big_bits):
    """The third base goes wide together with G and K (forced from the first item here, also with another width and switched off)."""
    monkeypatch.setenv("EG_COMB_BIG_MIN", "1")
    monkeypatch.setenv("EG_COMB_BIG_BITS", str(big_bits))
    c = eg.Context(0)
    try:
        v = eg.CommitmentEquivalenceVerifier(c, key, h, b"test")
        # scalars that exercise the window corners of both widths as commitment responses are beyond a prover; random items and
        # tampered twins go through all three combs of every equation
        its = items_of(v.prove(77, 0, [0, 1, 2**64 - 1] + list(range(3, 400))))
        for i in range(0, len(its), 5):
            its[i] = flip(its[i], (i * 97) % (8 * R.ITEM))
        packed = b"".join(its)
        want = R.verify_many(key, h, b"test", packed)
        assert v.verify(packed) == want
        assert v.verify(packed) == want                  # second call: the tables are there
        assert c.comb_table_bits() == (20, big_bits)
        v.close()
    finally:
        c.close()


def test_refused_arguments(eg, ctx, key, h):
    lib = eg._load()
    with pytest.raises(eg.EgError, match="identity"):
        eg.CommitmentEquivalenceVerifier(ctx, key, bytes(32), b"test")
    with pytest.raises(eg.EgError, match="not a valid"):
        eg.CommitmentEquivalenceVerifier(ctx, key, BAD_POINT_BYTES, b"test")
    with pytest.raises(eg.EgError, match="255"):
        eg.CommitmentEquivalenceVerifier(ctx, key, h, b"x" * 256)
    with pytest.raises(eg.EgError):                      # the key: rules of every params object
        eg.CommitmentEquivalenceVerifier(ctx, bytes(32), h, b"test")
    with pytest.raises(eg.EgError):
        eg.CommitmentEquivalenceVerifier(ctx, BAD_POINT_BYTES, h, b"test")
    out = C.c_void_p()
    BAD_ARG, BAD_PUBLIC_KEY = -3, -4                     # include/eg_hip.h: EG_ERR_BAD_ARG, EG_ERR_BAD_PUBLIC_KEY
    create = lib.eg_commit_equiv_params_create
    assert create(ctx._h, key, bytes(32), b"test", 4, C.byref(out)) == BAD_ARG and not out.value
    assert create(ctx._h, key, BAD_POINT_BYTES, b"test", 4, C.byref(out)) == BAD_ARG and not out.value
    assert create(ctx._h, bytes(32), h, b"test", 4, C.byref(out)) == BAD_PUBLIC_KEY and not out.value
    assert create(ctx._h, BAD_POINT_BYTES, h, b"test", 4, C.byref(out)) == BAD_PUBLIC_KEY and not out.value
    assert create(ctx._h, key, h, b"x" * 256, 256, C.byref(out)) == BAD_ARG
    assert create(ctx._h, None, h, b"test", 4, C.byref(out)) == BAD_ARG
    assert create(ctx._h, key, None, b"test", 4, C.byref(out)) == BAD_ARG
    assert create(ctx._h, key, h, None, 4, C.byref(out)) == BAD_ARG
    assert create(ctx._h, key, h, b"test", 4, None) == BAD_ARG
    assert create(None, key, h, b"test", 4, C.byref(out)) == BAD_ARG
    v = eg.CommitmentEquivalenceVerifier(ctx, key, h, b"test")
    z = eg.PublicKeyVerifier(ctx, key, eg.PublicKeyVerifier.ZERO)
    try:
        vals = (C.c_uint64 * 2)(1, 2)
        buf = C.create_string_buffer(2 * R.ITEM)
        assert lib.eg_commit_equiv_prove_batch(v._h, 1, 0, 2, 0, None, buf, None) != 0
        assert lib.eg_commit_equiv_prove_batch(v._h, 1, 0, 2, 0, vals, None, None) != 0
        assert lib.eg_commit_equiv_prove_batch(None, 1, 0, 2, 0, vals, buf, None) != 0
        assert lib.eg_commit_equiv_prove_batch_device(v._h, 1, 0, 2, 0, None, None, None, None) != 0
        assert lib.eg_commit_equiv_prove_batch(z._h, 1, 0, 2, 0, vals, buf, None) != 0          # a params object of another kind
        assert lib.eg_commit_equiv_prove_batch(v._h, 1, 0, 0, 0, None, None, None) == 0          # nothing to do
        assert lib.eg_verify_proof_batch(v._h, 2, None, None) != 0
        assert lib.eg_commit_equiv_prove_batch(v._h, 1, 0, 2, 0, vals, buf, None) == 0
        assert v.verify(buf.raw) == [0, 0]
    finally:
        v.close()
        z.close()


# ------------------------------------------------------------------ the table of H
def test_h_table_against_the_primitive_tier(eg, ctx, ver, h):
    """Value 0 makes C = [r_c]H, a product over the comb table of H alone, and the prover hands out r_c: 1 000 random scalars against
    eg_vartime_multi_mul_batch (Straus over the decoded point, no table)."""
    n = 1000
    packed, blind = ver.prove(86, 0, [0] * n, with_blindings=True)
    grp = eg.Ristretto(ctx)
    want, ok = grp.vartime_multi_mul(1, blind, h * n)
    assert set(ok) == {1}
    cs = b"".join(it[64:96] for it in items_of(packed))
    assert cs == want
    assert len({blind[32 * i : 32 * i + 32] for i in range(n)}) == n


# ------------------------------------------------------------------ existing kinds, before and after
def test_existing_proof_kinds_are_unchanged_by_a_commit_equiv_object(eg, oracle, key, h):
    c = eg.Context(0)
    try:
        k = oracle.PublicKey(key)
        rs = oracle.rng_from_u64(404)
        zs, bs = [], []
        for i in range(300):
            zs.append(bytearray(k.encrypt_zero(rs)))
            bs.append(bytearray(k.encrypt_bool(bool(i & 1), rs)))
            if i % 4 == 1:
                zs[-1][(i * 7) % 128] ^= 1
                bs[-1][(i * 11) % 160] ^= 2
        zb, bb = b"".join(map(bytes, zs)), b"".join(map(bytes, bs))
        # decryption shares of participant 0 of a 2-of-3 key
        rnd = random.Random(8)
        coeffs = [rnd.randrange(L) for _ in range(2)]
        share0 = (coeffs[0] + coeffs[1]) % L
        shared_key, part_key = oracle.point_mul_generator(R.sc(coeffs[0])), oracle.point_mul_generator(R.sc(share0))
        sh = []
        for i in range(60):
            ct_r = oracle.point_mul_generator(R.sc(rnd.randrange(L)))
            it = bytearray(ct_r + oracle.decryption_share_new(R.sc(share0), ct_r, 3, 2, shared_key, 0, rs))
            if i % 3 == 1:
                it[(i * 5) % 128] ^= 4
            sh.append(bytes(it))
        sb = b"".join(sh)
        z = eg.PublicKeyVerifier(c, key, eg.PublicKeyVerifier.ZERO)
        b = eg.PublicKeyVerifier(c, key, eg.PublicKeyVerifier.BOOL)
        s = eg.DecryptionShareVerifier(c, shared_key, 3, 2, 0, part_key)
        before = (z.verify_batch(zb), b.verify_batch(bb), s.verify_batch(sb))
        assert before[0] == [k.verify_zero(bytes(x)) for x in zs] and before[1] == [k.verify_bool(bytes(x)) for x in bs]
        assert before[2] == [oracle.decryption_share_verify(part_key, 3, 2, shared_key, 0, x) for x in sh]
        assert all(0 in v and any(v) for v in before)
        v = eg.CommitmentEquivalenceVerifier(c, key, h, b"test")
        mine = v.prove(1, 0, [5, 6, 7])
        assert v.verify(mine) == [0, 0, 0]
        assert (z.verify_batch(zb), b.verify_batch(bb), s.verify_batch(sb)) == before            # the object exists
        z2 = eg.PublicKeyVerifier(c, key, eg.PublicKeyVerifier.ZERO)                             # created after it
        assert z2.verify_batch(zb) == before[0]
        v.close()
        assert (z.verify_batch(zb), b.verify_batch(bb), s.verify_batch(sb)) == before            # and after it is gone
        for o in (z, b, s, z2):
            o.close()
    finally:
        c.close()
