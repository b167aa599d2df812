"""The two proof kinds that put a caller's label into Transcript::new - sum of squares (eg_sumsq_params_create) and commitment
equivalence (eg_commit_equiv_params_create) - through the shipped entries under labels of EVERY length 0..255
(tests/transcript_scripts.py: PROOF_LABEL_LENGTHS).  Every byte of label moves every later operation of every item's transcript by one
position of the 166-byte STROBE block; tests/test_transcript_positions_cpu.py proves with the position model that this set of lengths
takes both programs through every start position of every kind of operation.  Label bytes are random in 1..255 with at least one
>= 0x80 (the device reads labels through `const char*`).

The independent side is the oracle: oracle.verify_sumsq for the items the GPU prover makes, and the restatement of
tests/commit_equiv_ref.py (built on the oracle's primitives and its transcript) for commitment equivalence, whose items the GPU prover
has to reproduce byte for byte.

Cost, measured on an MI355X.  Creating and destroying one params object usually takes 3.5 ms for a sum of squares and about
10 ms for a commitment equivalence; proving 70 items takes 1 - 2 ms and verifying them 1.5 - 2.5 ms.  About once in a hundred
objects a creation stalls for 2.5 - 5 s (seen for both kinds, in every run; a mean over 20 commitment-equivalence objects that
held one stall came out as 121 ms).  The cause lies in engine creation, not in the transcript, and is not looked into here.  Two
objects per length (the label, and the label with its last byte changed) make all 256 lengths cost about 60 s for both kinds
together, half of it in six stalls.  Chosen set: ALL lengths 0..255 for both kinds, cut into 16 cases per n_values for the sum of
squares and 32 cases for the commitment equivalence: 58 of the 64 cases took 0.15 - 1.1 s, the six that met a stall 4.9 - 5.5 s."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import pytest

import commit_equiv_ref as R
import transcript_scripts as ts

pytestmark = pytest.mark.gpu

SUMSQ_CHUNKS, CEQUIV_CHUNKS = 16, 32
N_ITEMS = 70                      # lanes 0, 63, 64 and the last lane
MARKED = (0, 63, 64, N_ITEMS - 1)
SUMSQ_CHALLENGE = 12              # EG_ST_QV_CREDIT_EQUIV_CHALLENGE: ChallengeMismatch of the sum-of-squares proof


def chunk(k, chunks):
    ls = ts.PROOF_LABEL_LENGTHS
    per = (len(ls) + chunks - 1) // chunks
    return ls[per * k : per * (k + 1)]


def proof_label(n):
    return ts.label_bytes(n, 40)


def other_label(label):
    """the label with its last byte changed (and still no NUL)"""
    return label[:-1] + bytes([label[-1] ^ 0x01 or 0x81])


def flip(item, bit):
    t = bytearray(item)
    t[bit // 8] ^= 1 << (bit % 8)
    return bytes(t)


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


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(16) as ex:      # the oracle is a C library behind ctypes: the interpreter lock is released inside it
        yield ex


def test_the_sweep_covers_the_edges():
    for chunks in (SUMSQ_CHUNKS, CEQUIV_CHUNKS):
        all_lengths = [n for k in range(chunks) for n in chunk(k, chunks)]
        assert all_lengths == list(ts.PROOF_LABEL_LENGTHS) and all_lengths[0] == 0 and all_lengths[-1] == 255
    for n in all_lengths:
        label = proof_label(n)
        assert len(label) == n and 0 not in label and (n == 0 or max(label) >= 0x80)
        assert n == 0 or (other_label(label) != label and 0 not in other_label(label))


@pytest.mark.parametrize("n_values", [1, 2])
@pytest.mark.parametrize("k", range(SUMSQ_CHUNKS))
def test_sum_of_squares_under_labels_of_every_length(eg, ctx, oracle, pk, pool, n_values, k):
    key = oracle.PublicKey(pk)
    size = 64 * (n_values + 1) + 32 * (2 * n_values + 2)
    c_at = 64 * (n_values + 1)                       # the challenge follows the ciphertexts

    def oracle_status(label):
        return lambda it: key.verify_sumsq(it[: 64 * n_values], it[64 * n_values : c_at], it[c_at:], label)

    for n in chunk(k, SUMSQ_CHUNKS):
        label = proof_label(n)
        v = eg.SumOfSquaresVerifier(ctx, pk, n_values, label)
        try:
            assert v.item_size == size
            packed = v.prove(9000 + n, 0, [[(n + 3 * i + j) % 11 for j in range(n_values)] for i in range(N_ITEMS)])
            items = [packed[size * i : size * (i + 1)] for i in range(N_ITEMS)]
            # the prover's transcript, checked by the independent verifier, and the GPU verifier's
            assert list(pool.map(oracle_status(label), items)) == [0] * N_ITEMS, n
            twins = [flip(items[i], 8 * c_at + (37 * i + n) % 252) for i in MARKED]
            want = list(pool.map(oracle_status(label), twins))
            assert want == [SUMSQ_CHALLENGE] * len(MARKED), n
            assert v.verify_batch(packed + b"".join(twins)) == [0] * N_ITEMS + want, n
        finally:
            v.close()
        if n == 0:
            continue
        wrong = other_label(label)
        w = eg.SumOfSquaresVerifier(ctx, pk, n_values, wrong)
        try:
            got = w.verify_batch(packed)
            assert [got[i] for i in MARKED] == list(pool.map(oracle_status(wrong), [items[i] for i in MARKED])), n
            assert set(got) == {SUMSQ_CHALLENGE}, n
        finally:
            w.close()


@pytest.mark.parametrize("k", range(CEQUIV_CHUNKS))
def test_commitment_equivalence_under_labels_of_every_length(eg, ctx, oracle, k):
    fx = R.fixture()
    key, h = oracle.keypair_from_seed(fx["seed"])[1], bytes(fx["blinding_base"])
    values = [0, 2**64 - 1, 77]
    for n in chunk(k, CEQUIV_CHUNKS):
        label = proof_label(n)
        seed = 700 + n
        items = [R.prove(key, h, label, val, oracle.rng_from_u64(seed + i))[0] for i, val in enumerate(values)]
        assert [R.verify(key, h, label, it) for it in items] == [R.OK] * len(items), n
        twins = [flip(it, 8 * 96 + (41 * i + n) % 252) for i, it in enumerate(items)]            # bytes 96..127: the challenge
        want = [R.verify(key, h, label, t) for t in twins]
        assert want == [R.CHALLENGE] * len(twins), n
        v = eg.CommitmentEquivalenceVerifier(ctx, key, h, label)
        try:
            assert v.verify(b"".join(items + twins)) == [R.OK] * len(items) + want, n
            assert v.prove(seed, 0, values) == b"".join(items), n
        finally:
            v.close()
        if n == 0:
            continue
        wrong = other_label(label)
        w = eg.CommitmentEquivalenceVerifier(ctx, key, h, wrong)
        try:
            assert w.verify(b"".join(items)) == [R.verify(key, h, wrong, it) for it in items] == [R.CHALLENGE] * len(items), n
        finally:
            w.close()


def test_labels_that_are_refused(eg, ctx, oracle, pk):
    lib = eg._load()
    fx = R.fixture()
    h = bytes(fx["blinding_base"])
    BAD_ARG = -3                                      # include/eg_hip.h: EG_ERR_BAD_ARG
    out = C.c_void_p()
    long_label = ts.label_bytes(256, 41)
    assert lib.eg_sumsq_params_create(ctx._h, pk, 1, long_label, 256, C.byref(out)) == BAD_ARG and not out.value
    assert lib.eg_commit_equiv_params_create(ctx._h, pk, h, long_label, 256, C.byref(out)) == BAD_ARG and not out.value
    assert lib.eg_sumsq_params_create(ctx._h, pk, 1, None, 1, C.byref(out)) == BAD_ARG and not out.value
    assert lib.eg_commit_equiv_params_create(ctx._h, pk, h, None, 1, C.byref(out)) == BAD_ARG and not out.value
    # a NULL label of length 0 is the empty label
    assert lib.eg_sumsq_params_create(ctx._h, pk, 1, None, 0, C.byref(out)) == 0 and out.value
    try:
        v = eg.SumOfSquaresVerifier(ctx, pk, 1, b"")
        try:
            st = (C.c_uint32 * 1)()
            item = v.prove(1, 0, [[3]])
            assert lib.eg_verify_proof_batch(out, 1, item, st) == 0 and st[0] == 0
        finally:
            v.close()
    finally:
        lib.eg_proof_params_destroy(out)
