"""Ballot weeding (eg_*_weed[_device]) on the GPU.  The pass only compares bytes, so most cases are random bytes laid out as ballots,
with status NULL or hand-made status words, and every expected value comes from the model of the rule in tests/weed_ref.py.  The
end-to-end cases use ballots of the GPU generator: copies verify, weeding flags exactly the copies, and the grouped tally over the
weeded status words is the verify entry's tally of the originals alone."""
import statistics
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import weed_ref as W

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NONE, PRIOR, DUPLICATE = W.DUP_NONE, W.DUP_PRIOR, W.ST_DUPLICATE


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
def pk(oracle):
    return oracle.keypair_from_seed(12345)[1]


class Shape:
    """a params object, its oracle twin and the R items of its keys (found in a ballot of the oracle: the tally of one ballot is its keys)"""

    def __init__(self, eg, ctx, oracle, pk, kind, n_options, arg=0):
        self.kind, self.n_options = kind, n_options
        if kind == "qv":
            self.op, self.p = oracle.QvParams(pk, n_options, arg), eg.QuadraticVotingParams(ctx, pk, n_options, arg)
            one = self.op.generate_batch(5, 0, 1)
        else:
            self.op, self.p = oracle.ChoiceParams(pk, n_options, kind == "single"), eg.ChoiceParams(ctx, pk, n_options, kind == "single")
            one = self.op.generate_batch(5, 0, 1, arg) if arg else self.op.generate_batch(5, 0, 1)
        self.size = self.p.ballot_size
        keys = self.op.tally(one, [0])
        self.r_items = [one.index(keys[64 * k:64 * k + 64]) // 32 for k in range(n_options)]
        assert all(one[32 * r:32 * r + 64] == keys[64 * k:64 * k + 64] for k, r in enumerate(self.r_items))

    def random_ballots(self, seed, n):
        """n ballots of random bytes -> numpy [n, size]"""
        return np.random.default_rng(seed).integers(0, 256, (n, self.size), dtype=np.uint8)

    def keys(self, arr):
        return W.keys_of(arr.tobytes(), self.size, self.r_items)

    def copy_key(self, arr, dst, k_dst, src, k_src):
        arr[dst, 32 * self.r_items[k_dst]:32 * self.r_items[k_dst] + 64] = arr[src, 32 * self.r_items[k_src]:32 * self.r_items[k_src] + 64]


@pytest.fixture(scope="module")
def single5(eg, ctx, oracle, pk):
    return Shape(eg, ctx, oracle, pk, "single", 5)


def u32(torch, values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).cuda()


def as_u32(t):
    return [v & 0xFFFFFFFF for v in t.cpu().tolist()]


CANARY = 0x5C


def weed_dev(torch, shape, d_ballots, n, status=None, board=b"", board_cap=None, seed=0x1234567, append=False, alias=False, want_out=True,
             stream=0):
    """the device entry with buffers of its own (a canary behind the scratch and behind dup_of) -> dict"""
    p = shape.p
    n_prior = len(board) // 64
    board_cap = n_prior if board_cap is None else board_cap
    d_board = torch.full((max(board_cap, 1) * 64,), 0xEE, dtype=torch.uint8, device="cuda")
    if n_prior:
        d_board[: 64 * n_prior] = torch.frombuffer(bytearray(board), dtype=torch.uint8).cuda()
    need = p.weed_scratch_bytes(n, n_prior)
    scratch = torch.full((need + 64,), CANARY, dtype=torch.uint8, device="cuda")
    dup = torch.full((n + 16,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
    d_status = None if status is None else (status if hasattr(status, "data_ptr") else u32(torch, status))
    out = d_status if alias else torch.full((max(n, 1),), 0x77, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    found = torch.full((3,), 77, dtype=torch.int32, device="cuda")          # the library WRITES the three words
    torch.cuda.synchronize()
    p.weed_device(n, d_ballots.data_ptr() if n else 0, 0 if d_status is None else d_status.data_ptr(), n_prior, d_board.data_ptr(), board_cap,
                  seed, scratch.data_ptr() if need else 0, dup.data_ptr(), found.data_ptr(), d_status_out=out.data_ptr() if want_out else 0,
                  d_board_count=count.data_ptr() if append else 0, stream=stream)
    torch.cuda.synchronize()
    assert bytes(scratch[need:].cpu().numpy()) == bytes([CANARY]) * 64, "the pass wrote behind its scratch"
    assert dup[n:].cpu().tolist() == [0x5C5C5C5C] * 16, "the pass wrote behind dup_of"
    return dict(dup=as_u32(dup[:n]), out=as_u32(out[:n]) if want_out else None, found=tuple(found.cpu().tolist()), count=int(count.item()),
                board=bytes(d_board.cpu().numpy())[: 64 * board_cap])


def check_against_model(torch, shape, arr, status=None, board=(), **kw):
    got = weed_dev(torch, shape, dev(torch, arr), len(arr), status=status, board=b"".join(board), **kw)
    dup, out, appended = W.weed(shape.keys(arr), status, list(board))
    assert got["dup"] == dup
    assert got["out"] == out
    assert got["found"] == W.found(dup) + (0,)
    return got, dup, out, appended


# ------------------------------------------------------------------ sizes and lanes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_copies_at_the_seams_of_wavefronts_and_blocks(torch, single5, n):
    """the copy at lanes 0, 63, 64 and last: against the board (the only way ballot 0 is flagged), as a copy of the first ballot, and as
    the original of the last ballot; with 1025 ballots, a copy and an append across the first tile of the scan over the keep flags"""
    board = [bytes(np.random.default_rng(99).integers(0, 256, 64, dtype=np.uint8))]
    for at in sorted({0, 63, 64, n - 1}):
        if at >= n:
            continue
        arr = single5.random_ballots(n, n)
        arr[at, 32 * single5.r_items[3]:32 * single5.r_items[3] + 64] = np.frombuffer(board[0], dtype=np.uint8)
        got, dup, _, _ = check_against_model(torch, single5, arr, board=board)
        assert dup[at] == PRIOR and got["found"][:2] == (1, 0)
        if at > 0:
            arr = single5.random_ballots(n, n)
            arr[at] = arr[0]
            _, dup, _, _ = check_against_model(torch, single5, arr)
            assert dup[at] == 0 and dup.count(NONE) == n - 1
        if at < n - 1:
            arr = single5.random_ballots(n, n)
            arr[n - 1] = arr[at]
            _, dup, _, _ = check_against_model(torch, single5, arr)
            assert dup[n - 1] == at and dup.count(NONE) == n - 1
    arr = single5.random_ballots(n, n)
    _, dup, _, _ = check_against_model(torch, single5, arr)
    assert dup == [NONE] * n
    if n > 1024:                                                          # ballot 1024 copies ballot 1023; the kept keys go out in ballot order
        arr[1024] = arr[1023]
        _, _, appended = W.weed(single5.keys(arr), None, [])
        got, dup, _, _ = check_against_model(torch, single5, arr, board_cap=len(appended), append=True)
        assert dup[1024] == 1023 and dup.count(NONE) == n - 1
        assert got["count"] == len(appended) == 5 * (n - 1) and got["board"] == b"".join(appended) and got["found"][2] == 0


def test_4096_identical_ballots(torch, single5):
    arr = np.repeat(single5.random_ballots(1, 1), 4096, axis=0)
    got = weed_dev(torch, single5, dev(torch, arr), 4096)
    assert got["dup"] == [NONE] + [0] * 4095 and got["found"] == (0, 4095, 0)
    assert got["out"] == [0] + [DUPLICATE] * 4095


# ------------------------------------------------------------------ the rule
def planted_array(shape, seed, n, n_board):
    ballots, board = W.planted(seed, n, shape.n_options, n_board)
    arr = shape.random_ballots(seed, n)
    for b, keys in enumerate(ballots):
        for k, key in enumerate(keys):
            arr[b, 32 * shape.r_items[k]:32 * shape.r_items[k] + 64] = np.frombuffer(key, dtype=np.uint8)
    return arr, board


@pytest.mark.parametrize("n_board", [0, 1, 300])
def test_chain_cross_position_and_boards(torch, single5, n_board):
    """whole copies, one key at another option position, the chain A{x,y} B{y,z} C{z,w} (both B and C flagged), a key twice inside one
    ballot (no duplicate), a copy of a copy; boards of 0, 1 and 300 entries with hits (first and last entry) and misses"""
    arr, board = planted_array(single5, 21, 257, n_board)
    got, dup, _, _ = check_against_model(torch, single5, arr, board=board)
    assert (dup[20], dup[21], dup[22], dup[23]) == (NONE, 20, 21, 22) and dup[30] == NONE and dup[11] == 5 and dup[33] == 2
    if n_board:
        assert dup[3] == dup[35] == dup[36] == PRIOR and got["found"][0] == 3
    else:
        assert PRIOR not in dup


@pytest.mark.parametrize("kind,n_options,arg", [("single", 2, 0), ("multi", 16, 3), ("qv", 3, 4)])
def test_other_election_shapes(torch, eg, ctx, oracle, pk, kind, n_options, arg):
    """2 options, 3-of-16 multi-choice, quadratic voting with 3 options and 4 credits: the model on planted copies; for quadratic voting
    a copied partial or credit ciphertext - every 64 bytes of a ballot that are no key - is not flagged"""
    shape = Shape(eg, ctx, oracle, pk, kind, n_options, arg)
    try:
        arr, board = planted_array(shape, 31, 70, 4)
        check_against_model(torch, shape, arr, board=board)
        if kind == "qv":
            assert shape.r_items[1] - shape.r_items[0] > 2          # partial ciphertexts lie between two vote ciphertexts
            arr = shape.random_ballots(8, 40)
            key_bytes = {32 * r + i for r in shape.r_items for i in range(64)}
            free = [o for o in range(0, shape.size - 63, 32) if not key_bytes & set(range(o, o + 64))]
            assert len(free) >= 4
            for i, o in enumerate(free):
                arr[1 + i % 39, o:o + 64] = arr[0, o:o + 64]
            _, dup, _, _ = check_against_model(torch, shape, arr)
            assert dup == [NONE] * 40
            arr[17, 32 * shape.r_items[2]:32 * shape.r_items[2] + 64] = arr[0, 32 * shape.r_items[0]:32 * shape.r_items[0] + 64]
            _, dup, _, _ = check_against_model(torch, shape, arr)
            assert dup[17] == 0 and dup.count(NONE) == 39
    finally:
        shape.p.close()


def test_hand_made_status_words(torch, single5):
    """a rejected original does not own its keys; a rejected copy is EG_DUP_NONE and keeps its word; status_out both aliasing d_status
    and separate, and not wanted at all"""
    arr = single5.random_ballots(5, 130)
    status = [0] * 130
    for b in (0, 9, 64, 100):
        status[b] = 6 + (b << 8)
    arr[10], arr[70], arr[64], arr[129], arr[101] = arr[9], arr[10], arr[3], arr[100], arr[4]
    got, dup, out, _ = check_against_model(torch, single5, arr, status=status)
    assert dup[10] == NONE and dup[70] == 10 and dup[64] == NONE and out[64] == 6 + (64 << 8) and dup[129] == NONE and dup[101] == 4
    d_status = u32(torch, status)
    aliased = weed_dev(torch, single5, dev(torch, arr), 130, status=d_status, alias=True)
    assert aliased["dup"] == dup and aliased["out"] == out and as_u32(d_status) == out
    plain = weed_dev(torch, single5, dev(torch, arr), 130, status=status, want_out=False)
    assert plain["dup"] == dup and plain["found"] == got["found"]
    everyone, dup_all, _, _ = check_against_model(torch, single5, arr)          # status NULL: every ballot participates
    assert dup_all[10] == 9 and dup_all[70] == 9 and dup_all[64] == 3 and dup_all[129] == 100


# ------------------------------------------------------------------ append
def test_append_is_the_ballot_order_list(torch, single5):
    arr, board = planted_array(single5, 44, 300, 7)
    status = [0 if b % 11 else 4 for b in range(300)]
    _, _, appended = W.weed(single5.keys(arr), status, board)
    fit = 7 + len(appended)
    got, dup, _, _ = check_against_model(torch, single5, arr, status=status, board=board, board_cap=fit, append=True)
    assert got["count"] == fit and got["board"] == b"".join(board) + b"".join(appended)
    roomy, _, _, _ = check_against_model(torch, single5, arr, status=status, board=board, board_cap=fit + 9, append=True)
    assert roomy["count"] == fit and roomy["board"] == b"".join(board) + b"".join(appended) + b"\xee" * (64 * 9)
    # one entry too few: nothing is appended, the count stays, the bad word is set - the verdicts are the same
    short = weed_dev(torch, single5, dev(torch, arr), 300, status=status, board=b"".join(board), board_cap=fit - 1, append=True)
    assert short["dup"] == dup and short["found"] == W.found(dup) + (1,) and short["count"] == 7
    assert short["board"] == b"".join(board) + b"\xee" * (64 * (fit - 8))
    # no count pointer: no append, the board is untouched
    quiet = weed_dev(torch, single5, dev(torch, arr), 300, status=status, board=b"".join(board), board_cap=fit)
    assert quiet["dup"] == dup and quiet["count"] == -5 and quiet["board"] == b"".join(board) + b"\xee" * (64 * len(appended))


def test_three_seeds_and_n_zero(torch, single5):
    arr, board = planted_array(single5, 52, 257, 30)
    runs = [weed_dev(torch, single5, dev(torch, arr), 257, board=b"".join(board), board_cap=30 + 257 * 5, append=True, seed=s)
            for s in (0, 1, 0xFFFFFFFFFFFFFFFF)]
    assert runs[0] == runs[1] == runs[2] and runs[0]["found"][2] == 0
    empty = weed_dev(torch, single5, None, 0, board=b"".join(board), board_cap=40, append=True)
    assert empty["dup"] == [] and empty["found"] == (0, 0, 0) and empty["count"] == 30 and single5.p.weed_scratch_bytes(0, 30) == 0
    assert single5.p.weed(b"") == ([], [], None) and single5.p.weed(b"", None, b"".join(board), append=True) == ([], [], b"")


def test_entry_forms_agree_on_a_caller_stream_and_twice(torch, single5):
    arr, board = planted_array(single5, 61, 257, 12)
    status = [0 if b % 7 else 2 for b in range(257)]
    dup, out, appended = W.weed(single5.keys(arr), status, board)
    s = torch.cuda.Stream()
    d = dev(torch, arr)
    first = weed_dev(torch, single5, d, 257, status=status, board=b"".join(board), board_cap=12 + 257 * 5, append=True, stream=s.cuda_stream)
    second = weed_dev(torch, single5, d, 257, status=status, board=b"".join(board), board_cap=12 + 257 * 5, append=True)
    assert first == second and first["dup"] == dup and first["out"] == out
    for _ in range(2):
        assert single5.p.weed(arr.tobytes(), status, b"".join(board), append=True) == (dup, out, b"".join(appended))
    assert single5.p.weed(arr.tobytes(), status, b"".join(board)) == (dup, out, None)


def test_every_refusal_with_a_params_object(torch, eg, single5):
    p, n = single5.p, 64
    d = dev(torch, single5.random_ballots(2, n))
    scratch = torch.empty(p.weed_scratch_bytes(n, 4) + 16, dtype=torch.uint8, device="cuda")
    board = torch.zeros(64 * 400, dtype=torch.uint8, device="cuda")
    dup, found = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    good = dict(n=n, d_ballots=d.data_ptr(), d_status=0, n_prior=4, d_board=board.data_ptr(), board_cap=400, hash_seed=5,
                d_scratch=scratch.data_ptr(), d_dup_of=dup.data_ptr(), d_found=found.data_ptr(), d_board_count=count.data_ptr())
    p.weed_device(**good)
    torch.cuda.synchronize()
    assert found.cpu().tolist()[:3] == [0, 0, 0] and int(count.item()) == 4 + 5 * n
    for change, message in ((dict(n=1 << 31), "n is 2\\^31"), (dict(n_prior=1 << 31, board_cap=1 << 32), "n_prior is 2\\^31"),
                            (dict(n=(1 << 30) // 5, n_prior=5, board_cap=5), "EG_WEED_KEYS_MAX"), (dict(n_prior=401), "above board_cap"),
                            (dict(d_ballots=0), "null ballots"), (dict(d_dup_of=0), "null dup_of"), (dict(d_found=0), "null found"),
                            (dict(d_board=0), "null board"), (dict(d_board=0, n_prior=0), "null board with an append"),
                            (dict(d_scratch=0), "null scratch"), (dict(d_ballots=d.data_ptr() + 4), "aligned"),
                            (dict(d_board=board.data_ptr() + 8), "aligned"), (dict(d_scratch=scratch.data_ptr() + 8), "aligned")):
        with pytest.raises(eg.EgError, match=message):
            p.weed_device(**{**good, **change})
    assert p.weed_scratch_bytes(1 << 31, 0) == 0 == p.weed_scratch_bytes(1, 1 << 31) == p.weed_scratch_bytes((1 << 30) // 5, 5)
    assert p.weed_scratch_bytes(n, 4) == 8 * 1024 + 256 + 256 + 256          # 324 keys: 1024 slots; flags, one tile, the total
    torch.cuda.synchronize()


def test_passes_beside_a_verifying_thread(torch, single5):
    """two threads weed while a third verifies on the same params object: the pass takes no lock and touches no workspace"""
    p, n = single5.p, 2000
    d = torch.zeros(n * single5.size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(808, 0, n, d.data_ptr())
    p.ctx.synchronize()
    view = d.view(n, single5.size)
    view[1500:1520] = view[100:120]
    torch.cuda.synchronize()
    arr = view.cpu().numpy()
    dup, out, _ = W.weed(single5.keys(arr))
    assert dup.count(NONE) == n - 20 and dup[1500] == 100
    errors, results = [], {}

    def weeder(k):
        try:
            s = torch.cuda.Stream()
            results[k] = [weed_dev(torch, single5, d, n, seed=k + 3, stream=s.cuda_stream) for _ in range(3)]
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    def verifier():
        try:
            s = torch.cuda.Stream()
            st = torch.full((n,), 9, dtype=torch.int32, device="cuda")
            for _ in range(3):
                p.verify_batch_device(n, d.data_ptr(), st.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            results["status"] = st.cpu().tolist()
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=weeder, args=(0,)), threading.Thread(target=weeder, args=(1,)), threading.Thread(target=verifier)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    p.tally_reset()
    assert not errors, errors
    assert results["status"] == [0] * n                       # the copies verify
    for k in (0, 1):
        for run in results[k]:
            assert run["dup"] == dup and run["out"] == out and run["found"] == (0, 20, 0)


def test_large_batch_of_random_bytes_against_the_model(torch, single5):
    """2^17 + 3 ballots with 1 % planted copies (whole ballots, and single keys at another position), every ballot against the model"""
    n = (1 << 17) + 3
    arr = single5.random_ballots(1717, n)
    rng = np.random.default_rng(4)
    copies = rng.choice(np.arange(1, n), n // 100, replace=False)
    for i, b in enumerate(copies):
        src = int(rng.integers(0, b))
        if i % 3:
            arr[b] = arr[src]
        else:
            single5.copy_key(arr, b, i % 5, src, (i + 2) % 5)
    _, dup, _, _ = check_against_model(torch, single5, arr)
    assert n // 200 < sum(d != NONE for d in dup) <= n // 50          # (a source overwritten later leaves its earlier copy alone)


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def replayed(torch, single5):
    """300 valid ballots of the GPU generator and 20 whole copies behind them; everything verifies"""
    p, size = single5.p, single5.size
    d = torch.zeros(320 * size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(9090, 0, 300, d.data_ptr())
    p.ctx.synchronize()
    view = d.view(320, size)
    src = [(13 * i + 2) % 300 for i in range(20)]
    view[300:] = view[torch.tensor(src, device="cuda")]
    torch.cuda.synchronize()
    ballots = bytes(d.cpu().numpy())
    status, tally_all = p.verify_batch(ballots)
    _, tally_300 = p.verify_batch(ballots[: 300 * size])
    p.tally_reset()
    return dict(ballots=ballots, status=status, tally_all=tally_all, tally_300=tally_300, src=src)


def test_end_to_end_the_copies_verify_are_weeded_and_not_counted(single5, replayed):
    R, p = replayed, single5.p
    assert R["status"] == [0] * 320                                # today every copy is accepted ...
    assert R["tally_all"] != R["tally_300"]                        # ... and counted
    dup, out, appended = p.weed(R["ballots"], R["status"], append=True)
    assert dup == [NONE] * 300 + R["src"] and out == [0] * 300 + [DUPLICATE] * 20
    assert len(appended) == 300 * 5 * 64
    tallies, counts = p.tally_grouped(R["ballots"], out, [0] * 320, 1)
    assert counts == [300] and tallies == R["tally_300"]          # byte for byte the tally of the originals alone
    tallies, _, counts = p.tally_weighted(R["ballots"], out, [1] * 320, weight_bits=1)
    assert counts == [300] and tallies == R["tally_300"]


def test_end_to_end_through_the_board(single5, replayed):
    """batch 1 (ballots 0..199) appends to the board; batch 2 holds 100 new ballots and the 20 copies, of which those of batch 1 come
    back EG_DUP_PRIOR and those of batch 2 with their index in the batch"""
    R, p, size = replayed, single5.p, single5.size
    first, second = R["ballots"][: 200 * size], R["ballots"][200 * size:]
    dup1, out1, board = p.weed(first, [0] * 200, append=True)
    assert dup1 == [NONE] * 200 and len(board) == 200 * 5 * 64
    dup2, out2, more = p.weed(second, [0] * 120, board, append=True)
    want = [NONE] * 100 + [PRIOR if s < 200 else s - 200 for s in R["src"]]
    assert dup2 == want and PRIOR in want and any(d < 100 for d in want)
    assert len(more) == 100 * 5 * 64 and more == b"".join(b"".join(k) for k in single5.keys(np.frombuffer(second, dtype=np.uint8).reshape(120, size)[:100]))
    t1, c1 = p.tally_grouped(first, out1, [0] * 200, 1)
    t2, c2 = p.tally_grouped(second, out2, [0] * 120, 1)
    assert c1 == [200] and c2 == [100]
    p.tally_reset()
    p.tally_add(t1)
    p.tally_add(t2)
    assert p.tally_encode() == R["tally_300"]
    p.tally_reset()


def test_cpp_voting_example_with_replays(tmp_path):
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "voting.cpp"),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    out = subprocess.run([str(exe), "--replays", "5", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "99 of 100 ballots verified" in out.stdout and "with 5 replayed ballots: 104 of 105 ballots verified" in out.stdout
    assert "weeding dropped 5 ballots" in out.stdout and "the weeded totals equal those without the replays" in out.stdout
    assert "voter #101 dropped: repeats a ciphertext of voter #2" in out.stdout
    assert "OK: the decrypted totals equal the expected ones" in out.stdout
    out = subprocess.run([str(exe), "--qv", "--replays", "3", "40", "3", "20", "11"], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "weeding dropped 3 ballots" in out.stdout and "the weeded totals equal those without the replays" in out.stdout


# ------------------------------------------------------------------ a loose guard against a pass that has gone quadratic
def test_weeding_is_cheaper_than_verifying(torch, single5):
    """the pass over 2^16 five-option ballots takes less time than eg_verify_choice_batch_device on the same ballots in the same process
    (warm, median of three, HIP events).  Verification does about four orders of magnitude more arithmetic per ballot."""
    n, p = 1 << 16, single5.p
    d = torch.zeros(n * single5.size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(4242, 0, n, d.data_ptr())
    p.ctx.synchronize()
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    scratch = torch.empty(p.weed_scratch_bytes(n, 0), dtype=torch.uint8, device="cuda")
    dup = torch.zeros(n, dtype=torch.int32, device="cuda")
    found = torch.zeros(3, dtype=torch.int32, device="cuda")
    board = torch.zeros(n * 5 * 64, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        ms = []
        for _ in range(4):                       # the first round warms up
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms[1:])

    verify_ms = timed(lambda: p.verify_batch_device(n, d.data_ptr(), status.data_ptr(), stream=stream))
    weed_ms = timed(lambda: p.weed_device(n, d.data_ptr(), status.data_ptr(), 0, board.data_ptr(), n * 5, 77, scratch.data_ptr(), dup.data_ptr(),
                                          found.data_ptr(), d_board_count=count.data_ptr(), stream=stream))
    print(f"n = 2^16: weeding {weed_ms:.3f} ms, batch verify {verify_ms:.3f} ms")
    assert found.cpu().tolist() == [0, 0, 0] and int(status.abs().sum().item()) == 0 and int(count.item()) == n * 5
    assert as_u32(dup) == [NONE] * n
    assert weed_ms < verify_ms
    p.tally_reset()
