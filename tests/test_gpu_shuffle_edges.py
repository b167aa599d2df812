"""The shuffle verifier's chain kernel on the GPU where tests/test_gpu_shuffle.py does not reach (tests/shuffle_edge_cases.py has the
cases and the stated expectations, tests/test_shuffle_edges_cpu.py holds both against the oracle-judged model):
A  rows that PASS at edge scalars and edge points, built through a trapdoor key, with their off-by-one twins: the device against the
   model word for word, against the stated bits, and against the host build of the same header (tests/hostcheck/shufflecheck.cpp);
B  a wrong s^ at EVERY row of an honest proof of 190 rows, bad scalars and bad chain elements at the tiles' edges, sets of rows;
C  the sizes at which k_shuffle_fold and k_shuffle_chain take the second turn of their strided loops (65,541 rows; 63 rows for each of
   the 16 wavefronts of every CU, one tile and five rows), with proofs made by the model over the library's primitive tier and a
   sample of rows judged by the oracle;
D  eg_shuffle_key_derive_device, and a small verification in the scratch that a large one left behind."""
import random
import time

import pytest

import shuffle_cases as SC
import shuffle_edge_cases as E
import shuffle_ref as M
from test_gpu_shuffle import CANARY, MANY_TRIES_SEED, PAD, SK, Buf, run_device
from test_shuffle_cpu import check, run_verify  # noqa: F401  (the host build the device is compared with)
from test_shuffle_edges_cpu import CASES, N, check_case, edge_case, lanes_case, off_by_one_twins, row_sets, second_pass_rows

pytestmark = pytest.mark.gpu

FOLD_ROWS = 65536 + 5                       # 257 workgroups of scalars: the fold's second turn has one element
BIG_SEED = b"eg-shuffle second pass key"


@pytest.fixture(scope="module")
def eg():
    import elastic_elgamal_amd as m

    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


@pytest.fixture(scope="module")
def ctx(eg):
    c = eg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def be(oracle):
    return M.OracleBackend()


@pytest.fixture(scope="module")
def K(be):
    return be.mul_generator([SK])[0]


class Dev:
    """a statement resident on the device, verified with one proof after another in ONE scratch that is never cleared: canaries
    behind everything the library writes; (verdict, rows, found) per proof"""

    def __init__(self, eg, torch, ctx, t, scratch=None):
        self.torch, self.n, self.prefix = torch, len(t["ins"]), t["prefix"]
        n = self.n
        self.v = eg.ShuffleVerifier(ctx, t["K"], key=b"".join(t["key"][:n + 1]))
        self.need = self.v.verify_scratch_bytes(n)
        assert self.need > 0 and self.need % 256 == 0
        self.d_in, self.d_out, self.d_key = Buf(torch, b"".join(t["ins"])), Buf(torch, b"".join(t["outs"])), Buf(torch, self.v.key)
        self.d_verdict, self.d_found, self.d_rows = Buf(torch, size=4), Buf(torch, size=16), Buf(torch, size=4 * n)
        self.scratch = scratch if scratch is not None else torch.empty(self.need + PAD, dtype=torch.uint8, device="cuda")
        assert self.scratch.numel() >= self.need + PAD and self.scratch.data_ptr() % 256 == 0
        self.scratch[self.need:self.need + PAD] = CANARY

    def run(self, proof):
        torch, n = self.torch, self.n
        d_proof = Buf(torch, proof)
        self.v.verify_device(n, self.d_in.ptr, self.d_out.ptr, self.d_key.ptr, d_proof.ptr, self.d_verdict.ptr, self.d_found.ptr,
                             self.scratch.data_ptr(), self.need, prefix=self.prefix, d_rows=self.d_rows.ptr)
        torch.cuda.synchronize()
        for b in (self.d_verdict, self.d_found, self.d_rows, self.d_in, self.d_out, self.d_key, d_proof):
            assert b.intact()
        assert self.scratch[self.need:self.need + PAD].cpu().numpy().tobytes() == bytes([CANARY]) * PAD
        return self.d_verdict.words()[0], self.d_rows.words(), self.d_found.words()


# ------------------------------------------------------------------ A: passing rows at the edges
@pytest.mark.parametrize("k", range(CASES))
def test_edge_rows_pass_and_their_neighbours_in_value_fail(eg, torch, ctx, be, K, k):
    """case k of the placement (tests/test_shuffle_edges_cpu.py::test_placement): the built rows pass CHAIN on the device, s^ + 1 fails
    every row, s' + 1 in every second row fails exactly those, and verdict, rows and found are the oracle-judged model's"""
    t = edge_case(be, K, k)
    check_case(be, t, lambda twin: run_device(eg, torch, ctx, twin))


def test_edge_rows_through_the_host_entry(eg, ctx, be, K):
    t = edge_case(be, K, 1)
    v = eg.ShuffleVerifier(ctx, K, key=b"".join(t["key"]))
    check_case(be, t, lambda twin: v.verify(b"".join(twin["ins"]), b"".join(twin["outs"]), twin["proof"], twin["prefix"]))


def test_edge_rows_device_and_host_build_agree(check, eg, torch, ctx, be, K, tmp_path):  # noqa: F811
    """two compilations of one header on the same files: the kernels, and the lane functions of the host check under the sanitizers"""
    for k in (0, 1):
        t = lanes_case(be, K, k)
        a, b, _ = off_by_one_twins(t)
        for j, twin in enumerate((E.twin_of(t), a, b)):
            lanes = run_verify(check, tmp_path, twin, f"_gpu{k}{j}")
            assert run_device(eg, torch, ctx, twin) == lanes == SC.judge(be, twin), (k, twin["name"])
        check_case(be, t, lambda twin: run_device(eg, torch, ctx, twin))


# ------------------------------------------------------------------ B: every row position
@pytest.fixture(scope="module")
def honest(eg, torch, ctx, be, K):
    """an honest proof of N = 190 rows, made once by the model over the oracle and accepted by it; resident on the device"""
    key = M.derive_key(be, SC.SEED, N)
    base = SC.base(M.make(be, K, key, SC.PREFIX, N, 41000), K, key)
    assert SC.judge(be, base) == (0, [0] * N, E.NONE4)
    return base, Dev(eg, torch, ctx, base)


def test_a_wrong_shat_at_every_row(honest):
    base, dev = honest
    assert dev.run(base["proof"]) == (0, [0] * N, E.NONE4)
    for k in range(N):
        got = dev.run(E.with_rows(base, "", "shat", [k])["proof"])
        assert got == E.expect_shat_plus_one(N, [k]) == (M.CHAIN, [M.ROW_CHAIN if i == k else 0 for i in range(N)], [0, 1, M.NONE, k]), k


def test_bad_scalars_and_chain_elements_at_the_tiles_edges(honest):
    base, dev = honest
    assert E.edge_rows(N) == [0, 61, 62, 63, 64, 125, 126, N - 1]
    for k in E.edge_rows(N):
        for sec in ("sprime", "shat"):
            got = dev.run(E.with_rows(base, "", sec, [k], E.LL)["proof"])
            assert got == E.expect_scalar_is_l(N, k), (sec, k)
            assert got[0] == M.BAD_ENCODING and got[1][k] == M.ROW_BAD and got[2][0] == 1 and got[2][2] == k
        got = dev.run(E.with_rows(base, "", "chat", [k], SC.NOT_A_POINT)["proof"])
        assert got == E.expect_chat_not_a_point(N, k), k
        assert got[1][k] == M.ROW_BAD and (k + 1 == N or got[1][k + 1] == 0)


def test_sets_of_rows_count_exactly(honest):
    """all last lanes of the tiles, then all first lanes: the counts and minima of found under concurrent atomics"""
    base, dev = honest
    for name, rows in row_sets(N).items():
        assert len(rows) in (3, 4)
        assert dev.run(E.with_rows(base, name, "shat", rows)["proof"]) == E.expect_shat_plus_one(N, rows), name
    every = list(range(N))
    assert dev.run(E.with_rows(base, "all", "shat", every)["proof"]) == (M.CHAIN, [M.ROW_CHAIN] * N, [0, N, M.NONE, 0])


# ------------------------------------------------------------------ C: the second turn of the two strided loops
_big = {}


def big_world(eg, ctx, be, cus):
    """the maker, the key for the larger size (the library's; its first generators are held against the model's) and the election key"""
    if not _big:
        n = second_pass_rows(cus)
        raw = eg.ShuffleVerifier.derive_key(ctx, BIG_SEED, n)
        key = [raw[32 * j:32 * j + 32] for j in range(n + 1)]
        assert key[:40] == M.derive_key(be, BIG_SEED, 39)
        _big.update(maker=M.LibraryBackend(ctx), key=key, K=be.mul_generator([SK])[0])
    return _big


def big_case(eg, torch, ctx, be, n, seed, scratch=None):
    """(twin, Dev, x, seconds the prover took): an honest shuffle of n rows made by the model over the library's primitive tier"""
    w = big_world(eg, ctx, be, torch.cuda.get_device_properties(0).multi_processor_count)
    t0 = time.time()
    case = M.make(w["maker"], w["K"], w["key"], SC.PREFIX, n, seed)
    took = time.time() - t0
    base = SC.base(case, w["K"], w["key"][:n + 1])
    t, _, (c, chat, that, _, _) = M.split_proof(n, base["proof"])
    seed1, _ = M.challenges_u(n, base["ins"], base["outs"], base["K"], base["key"], SC.PREFIX, c)
    return base, Dev(eg, torch, ctx, base, scratch), M.challenge_x(n, seed1, chat, that, t), took


def judged_sample(be, base, x, proof, rows):
    """the row words of `rows` by the rule, the oracle evaluating: {row: word}.  The statement and the chain are the honest ones (every
    point decodes); only s^ and s' of `proof` differ from it, and x reads neither."""
    n = len(base["ins"])
    rows = sorted(set(rows))
    chat = lambda i: SC.get(proof, n, "chat", i) if i >= 0 else base["key"][0]
    assert all(be.decodes([chat(i) for i in rows] + [chat(i - 1) for i in rows]))
    words, ev, scalars, points = {}, [], [], []
    for i in rows:
        shat, sprime = E.scalar_of(proof, n, "shat", i), E.scalar_of(proof, n, "sprime", i)
        words[i] = 0 if shat < M.L and sprime < M.L else M.ROW_BAD
        if not words[i]:
            ev.append(i)
            scalars += [-x, sprime, shat]
            points += [chat(i), chat(i - 1), be.G]
    for i, got in zip(ev, be.multi_mul(3, scalars, points)):
        if got != SC.get(proof, n, "that", i):
            words[i] |= M.ROW_CHAIN
    return words


def sample_of(n, tampered, seed):
    """64 rows: the tampered ones, their neighbours, and seeded random rows"""
    near = {i + d for i in tampered for d in (-1, 0, 1) if 0 <= i + d < n}
    others = [i for i in random.Random(seed).sample(range(n), 128) if i not in near]
    return sorted(near | set(others[:64 - len(near)]))


def test_fold_second_turn(eg, torch, ctx, be):
    """257 partial products: the honest proof is accepted, and one flipped bit of s2 gives exactly T2 - the product of all u_i, which
    the fold makes, feeds T2 alone, and the bit is live at this size"""
    n = FOLD_ROWS
    assert -(-n // 256) == 257
    base, dev, x, took = big_case(eg, torch, ctx, be, n, 51000)
    print(f"prover: {took:.1f} s for {n} rows; scratch {dev.need / 1e6:.1f} MB")
    assert dev.run(base["proof"]) == (0, [0] * n, E.NONE4)
    s2 = SC.get(base["proof"], n, "s2")
    assert int.from_bytes(SC.flip(s2, 0, 2), "little") < M.L
    assert dev.run(SC.put(base["proof"], n, "s2", 0, SC.flip(s2, 0, 2))) == (M.T2, [0] * n, E.NONE4)
    got = dev.run(E.with_rows(base, "", "shat", [0, 65535, 65536, n - 1])["proof"])
    assert got == E.expect_shat_plus_one(n, [0, 65535, 65536, n - 1])
    del dev
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def second_pass(eg, torch, ctx, be):
    """the honest shuffle of 63 * 16 * CUs + 68 rows, verified once; its scratch serves every later proof of the module"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = second_pass_rows(cus)
    base, dev, x, took = big_case(eg, torch, ctx, be, n, 52000)
    print(f"prover: {took:.1f} s for {n} rows on {cus} CUs; scratch {dev.need / 1e6:.1f} MB")
    first = dev.run(base["proof"])
    yield base, dev, x, 63 * 16 * cus, first
    del dev
    torch.cuda.empty_cache()


def test_chain_second_turn(second_pass, be):
    """every wavefront of the capped grid has had its tile when rows `first` .. N - 1 are still to do: one full tile and one of five
    rows, taken by the first two wavefronts in a second turn of the loop, in the workspace tables they used before"""
    base, dev, x, first, honest_answer = second_pass
    n = dev.n
    assert n - first == 68 and honest_answer == (0, [0] * n, E.NONE4)
    both = [0, first // 2 + 17, first - 1, first, first + 30, n - 1]
    later = [first, first + 30, first + 63 + 2, n - 1]
    bad = first + 40
    for name, rows, found in (("both_passes", both, [0, 6, M.NONE, 0]), ("second_pass_only", later, [0, 4, M.NONE, first])):
        proof = E.with_rows(base, name, "shat", rows)["proof"]
        got = dev.run(proof)
        assert got == E.expect_shat_plus_one(n, rows) and got[0] == M.CHAIN and got[2] == found, name
        sample = sample_of(n, rows, 53000)
        assert len(sample) == 64
        assert {i: got[1][i] for i in sample} == judged_sample(be, base, x, proof, sample), name
    proof = E.with_rows(base, "sprime_is_l", "sprime", [bad], E.LL)["proof"]
    got = dev.run(proof)
    assert got == E.expect_scalar_is_l(n, bad) and got[0] == M.BAD_ENCODING and got[2] == [1, 0, bad, M.NONE]
    sample = sample_of(n, [bad], 53001)
    assert {i: got[1][i] for i in sample} == judged_sample(be, base, x, proof, sample)
    # the honest proof once more, judged at a sample: rows of both passes pass by the rule
    sample = sample_of(n, both + later, 53002)
    assert set(judged_sample(be, base, x, base["proof"], sample).values()) == {0}


# ------------------------------------------------------------------ D: small things
def test_a_small_verification_in_the_scratch_of_a_large_one(second_pass, eg, torch, ctx, be, K):
    """the same verifier object and the same scratch, left as the large call wrote it, with 65 rows: the model's answers"""
    base, dev, *_ = second_pass
    n = 65
    c = M.make(be, K, base["key"][:n + 1], SC.PREFIX, n, 54000)
    small = SC.base(c, K, base["key"][:n + 1])
    lie = E.with_rows(small, "shat_plus_one", "shat", [0, 62, 63, 64])
    d_in, d_out, d_proof, d_lie = Buf(torch, b"".join(small["ins"])), Buf(torch, b"".join(small["outs"])), Buf(torch, small["proof"]), Buf(torch, lie["proof"])
    d_verdict, d_found, d_rows = Buf(torch, size=4), Buf(torch, size=16), Buf(torch, size=4 * n)
    need = dev.v.verify_scratch_bytes(n)
    dev.scratch[need:need + PAD] = CANARY
    for twin, d_p in ((small, d_proof), (lie, d_lie)):
        dev.v.verify_device(n, d_in.ptr, d_out.ptr, dev.d_key.ptr, d_p.ptr, d_verdict.ptr, d_found.ptr, dev.scratch.data_ptr(), need,
                            prefix=SC.PREFIX, d_rows=d_rows.ptr)
        torch.cuda.synchronize()
        assert (d_verdict.words()[0], d_rows.words(), d_found.words()) == SC.judge(be, twin), twin["name"]
        assert all(b.intact() for b in (d_verdict, d_found, d_rows))
        assert dev.scratch[need:need + PAD].cpu().numpy().tobytes() == bytes([CANARY]) * PAD
    assert SC.judge(be, small) == (0, [0] * n, E.NONE4) and SC.judge(be, lie)[2] == [0, 4, M.NONE, 0]


@pytest.mark.parametrize("cap", [0, 255, 256, 257])
def test_key_derivation_on_the_device(eg, torch, ctx, be, K, cap):
    """eg_shuffle_key_derive_device: the model's generators and the host entry's, nothing behind generator `cap` (the lanes j > cap of
    the last workgroup write nothing), the exhausted word 0"""
    v = eg.ShuffleVerifier(ctx, K, key=bytes(32))
    for seed in (SC.SEED, MANY_TRIES_SEED, b""):
        d_key, d_ex = Buf(torch, size=32 * (cap + 1)), Buf(torch, data=b"\xff\xff\xff\xff")
        v.derive_key_device(seed, cap, d_key.ptr, d_ex.ptr)
        torch.cuda.synchronize()
        assert d_key.bytes() == b"".join(M.derive_key(be, seed, cap)) == eg.ShuffleVerifier.derive_key(ctx, seed, cap), (seed, cap)
        assert d_ex.words() == [0] and d_key.intact() and d_ex.intact()
