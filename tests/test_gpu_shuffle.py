"""The shuffle verifier (eg_shuffle_*) on the GPU.  Shuffles and proofs are made by the model tests/shuffle_ref.py over the library's
primitive tier; every expected verdict, row word and found word is the model's with the oracle backend judging, compared word for word.
The sizes cross the wavefront and the chain kernel's 63-row tiling (62 .. 65, 126 .. 128), the workgroup (255 .. 257), the eight-term
chunk of the product lane at 2N terms, the 1024-leaf tile of the tree and its second launch (1023 .. 1025, 2049).  Every size runs every
twin of tests/shuffle_cases.py.  The judge's verdicts of a size are computed once, kept at module level and left unchanged; a twin costs
the judge about a second at 2049 rows, so the twins of a size are judged on a few threads (the oracle's calls release the interpreter
lock and keep no state between calls)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import shuffle_cases as SC
import shuffle_ref as M

pytestmark = pytest.mark.gpu

CANARY, PAD = 0x5C, 256
SIZES = [1, 2, 3, 4, 5, 8, 9, 62, 63, 64, 65, 126, 127, 128, 255, 256, 257, 1023, 1024, 1025, 2049]
JUDGES = max(1, min(8, os.cpu_count() or 1))
CAP = 2060                                  # the key serves every size here: key_cap > N throughout
SK = 0x1F2E3D4C5B6A79880123456789ABCDEF % M.L
MANY_TRIES_SEED = b"eg-shuffle many tries 0"        # generators 1, 2 and 3 need 21, 30 and 26 candidates (tests/test_shuffle_cpu.py pins them)


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


class Buf:
    """device bytes with canaries behind"""

    def __init__(self, torch, data=None, size=None):
        self.size = len(data) if data is not None else size
        a = np.full(self.size + PAD, CANARY, dtype=np.uint8)
        if data:
            a[:self.size] = np.frombuffer(data, dtype=np.uint8)
        self.t = torch.from_numpy(a).cuda()
        self.ptr = self.t.data_ptr()

    def bytes(self):
        return self.t.cpu().numpy().tobytes()[:self.size]

    def words(self):
        return np.frombuffer(self.bytes(), dtype=np.uint32).tolist()

    def intact(self):
        return self.t.cpu().numpy().tobytes()[self.size:] == bytes([CANARY]) * PAD


_world = {}


@pytest.fixture(scope="module")
def world(ctx, oracle):
    """the judge, the maker, the election key and the commitment key (the model's, derived once)"""
    if not _world:
        judge, maker = M.OracleBackend(), M.LibraryBackend(ctx)
        _world.update(judge=judge, maker=maker, K=judge.mul_generator([SK])[0], key=M.derive_key(judge, SC.SEED, CAP), cases={})
    return _world


def cases_of(world, n):
    """(honest case, [(twin, the model's (mask, rows, found))]) of a size: made once, left unchanged"""
    if n not in world["cases"]:
        K, key, maker, judge = world["K"], world["key"], world["maker"], world["judge"]
        case = M.make(maker, K, key, SC.PREFIX, n, 9000 + n)
        twins = [SC.base(case, K, key)] + SC.tampered(case, K, key) + SC.lying(maker, case, K, key, 9000 + n)
        with ThreadPoolExecutor(JUDGES) as pool:
            world["cases"][n] = (case, list(zip(twins, pool.map(lambda t: SC.judge(judge, t), twins))))
    return world["cases"][n]


def run_device(eg, torch, ctx, t, want_rows=True, key_cap=None):
    """eg_shuffle_verify_device on a twin: (verdict, rows or None, found), with canaries behind every array the library writes"""
    n = len(t["ins"])
    key_cap = len(t["key"]) - 1 if key_cap is None else key_cap
    v = eg.ShuffleVerifier(ctx, t["K"], key=b"".join(t["key"][:key_cap + 1]))
    need = v.verify_scratch_bytes(n)
    assert need > 0 and need % 256 == 0
    d_in, d_out = Buf(torch, b"".join(t["ins"])), Buf(torch, b"".join(t["outs"]))
    d_key, d_proof = Buf(torch, v.key), Buf(torch, t["proof"])
    d_verdict, d_found, d_rows, d_scratch = Buf(torch, size=4), Buf(torch, size=16), Buf(torch, size=4 * n), Buf(torch, size=need)
    v.verify_device(n, d_in.ptr, d_out.ptr, d_key.ptr, d_proof.ptr, d_verdict.ptr, d_found.ptr, d_scratch.ptr, need, prefix=t["prefix"],
                    d_rows=d_rows.ptr if want_rows else 0)
    torch.cuda.synchronize()
    for b in (d_verdict, d_found, d_rows, d_scratch, d_in, d_out, d_key, d_proof):
        assert b.intact()
    if not want_rows:
        assert d_rows.bytes() == bytes([CANARY]) * (4 * n)
    return d_verdict.words()[0], d_rows.words() if want_rows else None, d_found.words()


@pytest.mark.parametrize("n", SIZES)
def test_verdicts_rows_and_found_equal_the_model(eg, torch, ctx, world, n):
    case, twins = cases_of(world, n)
    assert twins[0][1] == (0, [0] * n, [0, 0, M.NONE, M.NONE])                        # the judge accepts the honest proof
    seen = 0
    for t, want in twins:
        got = run_device(eg, torch, ctx, t)
        assert got == want, (n, t["name"], got[0], want[0], got[2], want[2])
        seen |= want[0]
    assert seen == 127 and len(twins) == 42 - (n < 2)                                        # every twin at every size; they meet every bit of the verdict
    honest, first_lie = twins[0][0], next(t for t, _ in twins if t["name"] == "that_flip")
    # rows == NULL; a key of exactly N + 1 generators; the host entry against the device entry
    assert run_device(eg, torch, ctx, honest, want_rows=False) == (0, None, [0, 0, M.NONE, M.NONE])
    assert run_device(eg, torch, ctx, honest, key_cap=n)[0] == 0
    for t in (honest, first_lie, twins[1][0]):
        v = eg.ShuffleVerifier(ctx, t["K"], key=b"".join(t["key"]))
        host = v.verify(b"".join(t["ins"]), b"".join(t["outs"]), t["proof"], t["prefix"])
        assert host == run_device(eg, torch, ctx, t)
        assert v.verify(b"".join(t["ins"]), b"".join(t["outs"]), t["proof"], t["prefix"], want_rows=False)[::2] == host[::2]


def test_single_bits(world):
    """what the lying provers must give, stated and not only mirrored: a wrong t^_k with its own challenge fails CHAIN in row k alone,
    another message in one output fails T41 alone, two rows on one generator fail T1 and / or T3 alone"""
    for n in (5, 64, 65):
        for t, (mask, rows, found) in cases_of(world, n)[1]:
            if t["name"] == "that_flip":
                assert mask == M.CHAIN and rows == [M.ROW_CHAIN if i == t["row"] else 0 for i in range(n)] and found == [0, 1, M.NONE, t["row"]]
            if t["name"] == "other_message":
                assert mask == M.T41 and not any(rows)
            if t["name"] == "two_on_one_H":
                assert mask and not mask & ~(M.T1 | M.T3) and not any(rows)


def test_empty_shuffle(eg, ctx, world):
    v = eg.ShuffleVerifier(ctx, world["K"], key=b"".join(world["key"]))
    assert v.verify(b"", b"", bytes(288), SC.PREFIX) == (0, [], [0, 0, M.NONE, M.NONE])


def test_key_derivation_equals_the_model(eg, ctx, world):
    assert eg.ShuffleVerifier.derive_key(ctx, SC.SEED, CAP) == b"".join(world["key"])
    assert eg.ShuffleVerifier.derive_key(ctx, SC.SEED, 0) == world["key"][0]                 # H_j does not depend on cap
    key, used = M.derive_key(world["judge"], MANY_TRIES_SEED, 8, with_tries=True)
    assert used[1:4] == [21, 30, 26]
    assert eg.ShuffleVerifier.derive_key(ctx, MANY_TRIES_SEED, 8) == b"".join(key)
    assert eg.ShuffleVerifier.derive_key(ctx, b"", 3) == b"".join(M.derive_key(world["judge"], b"", 3))


def test_two_mixers_then_decryption(eg, torch, ctx, world):
    """a cascade: mixer 2 shuffles what mixer 1 put out, both proofs are accepted, and the last outputs decrypt (eg_combine_shares_batch,
    one participant holding the whole key) to the input plaintexts as a multiset"""
    from elastic_elgamal_amd import tally

    n, K, key, maker = 65, world["K"], world["key"], world["maker"]
    first = cases_of(world, n)[0]
    import random

    rng = random.Random(77)
    src = list(range(n))
    rng.shuffle(src)
    rho = [rng.getrandbits(512) % M.L for _ in range(n)]
    outs2 = M.shuffle(maker, first["outs"], K, src, rho)
    proof2 = M.prove(maker, first["outs"], outs2, K, key, b"election-7/mixer-2", src, rho, rng)
    v = eg.ShuffleVerifier(ctx, K, key=b"".join(key))
    assert v.verify(b"".join(first["ins"]), b"".join(first["outs"]), first["proof"], SC.PREFIX)[0] == 0
    assert v.verify(b"".join(first["outs"]), b"".join(outs2), proof2, b"election-7/mixer-2")[0] == 0
    assert v.verify(b"".join(first["outs"]), b"".join(outs2), proof2, SC.PREFIX)[0] != 0     # not under the first mixer's prefix
    dh = maker.double_mul_generator([SK] * n, [o[:32] for o in outs2], [0] * n)
    items = b"".join(o[:32] + d + bytes(64) for o, d in zip(outs2, dh))
    _, plain, combined, _ = tally.combine_shares_batch(eg.Ristretto(ctx), 1, 1, b"".join(outs2), [0], items)
    assert bytes(combined) == b"\x01" * n
    want = maker.mul_generator(first["msgs"])
    assert sorted(plain[32 * i:32 * i + 32] for i in range(n)) == sorted(want)
