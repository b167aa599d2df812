"""Weeding against a persistent board index (eg_weed_index_*, eg_*_weed_indexed_device) on the GPU.  Every step of a chain of batches is
run twice - through eg_*_weed_device over a copy of the same board bytes and through the indexed pass over the board and its index -
and both are compared with each other, byte for byte, and with the model of the rule in tests/weed_ref.py.  Every buffer the passes
write has a canary behind it: scratch, index, board, dup_of and pos."""
import statistics
import subprocess
from pathlib import Path

import numpy as np
import pytest

import weed_ref as W

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NONE, PRIOR, DUPLICATE = W.DUP_NONE, W.DUP_PRIOR, W.ST_DUPLICATE
CANARY = 0x5C
INDEX_SEED = 0x0BADC0DE5EEDF00D


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
        return np.random.default_rng(seed).integers(0, 256, (n, self.size), dtype=np.uint8)

    def keys(self, arr):
        return W.keys_of(arr.tobytes(), self.size, self.r_items)

    def key_slice(self, k):
        return slice(32 * self.r_items[k], 32 * self.r_items[k] + 64)


@pytest.fixture(scope="module")
def single5(eg, ctx, oracle, pk):
    return Shape(eg, ctx, oracle, pk, "single", 5)


def u32(torch, values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def as_u32(t):
    return [v & 0xFFFFFFFF for v in t.cpu().tolist()]


def random_keys(seed, n):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, 64, dtype=np.uint8)) for _ in range(n)]


class Chain:
    """a board with room for `cap` ciphertexts in device memory, its index, and the model's copy of the board"""

    def __init__(self, torch, ctx, shape, start, cap, index_seed=INDEX_SEED):
        self.torch, self.ctx, self.shape, self.cap, self.index_seed = torch, ctx, shape, cap, index_seed
        self.model = list(start)
        self.board = torch.full((cap * 64 + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        if start:
            self.board[: 64 * len(start)] = torch.frombuffer(bytearray(b"".join(start)), dtype=torch.uint8).cuda()
        self.board[cap * 64:] = CANARY
        self.index_bytes = ctx.weed_index_bytes(cap)
        slots = 1024
        while slots < 2 * cap:
            slots *= 2
        assert self.index_bytes == 4 * slots
        self.index = self.new_index(index_seed)

    @property
    def n_prior(self):
        return len(self.model)

    def new_index(self, seed, board=None, n_prior=None):
        """eg_weed_index_build_device over the board as it is now, into fresh memory"""
        torch = self.torch
        index = torch.full((self.index_bytes + 64,), CANARY, dtype=torch.uint8, device="cuda")
        found = torch.full((2,), 77, dtype=torch.int32, device="cuda")
        self.ctx.weed_index_build_device(self.n_prior if n_prior is None else n_prior, (self.board if board is None else board).data_ptr(), self.cap,
                                         seed, index.data_ptr(), found.data_ptr())
        torch.cuda.synchronize()
        assert found.cpu().tolist() == [0, 77]
        assert bytes(index[self.index_bytes:].cpu().numpy()) == bytes([CANARY]) * 64, "build wrote behind the index"
        return index

    def find(self, queries, index=None, seed=None):
        """eg_weed_index_find_device over a list of 64-byte keys -> positions"""
        torch, n_q = self.torch, len(queries)
        keys = torch.frombuffer(bytearray(b"".join(queries) or b"\0"), dtype=torch.uint8).cuda()
        pos = torch.full((n_q + 16,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
        index = self.index if index is None else index
        before = index.clone()
        self.ctx.weed_index_find_device(n_q, keys.data_ptr(), self.n_prior, self.board.data_ptr(), self.cap, index.data_ptr(),
                                        self.index_seed if seed is None else seed, pos.data_ptr())
        torch.cuda.synchronize()
        assert pos[n_q:].cpu().tolist() == [0x5C5C5C5C] * 16, "find wrote behind pos"
        assert torch.equal(index, before), "find wrote into the index"
        return as_u32(pos[:n_q])

    def _pass(self, indexed, d_ballots, n, status, board, append, alias, want_out, seed, stream):
        torch, p = self.torch, self.shape.p
        need = p.weed_indexed_scratch_bytes(n) if indexed else p.weed_scratch_bytes(n, self.n_prior)
        if indexed:
            assert need == p.weed_scratch_bytes(n, 0)                      # a function of n alone: what the stateless pass needs beside no board
        scratch = torch.full((need + 64,), CANARY, dtype=torch.uint8, device="cuda")
        dup = torch.full((n + 16,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
        d_status = None if status is None else u32(torch, status)
        out = d_status if alias else torch.full((max(n, 1),), 0x77, dtype=torch.int32, device="cuda")
        count = torch.full((1,), -5, dtype=torch.int64, device="cuda")
        found = torch.full((4,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        common = dict(d_status_out=out.data_ptr() if want_out else 0, d_board_count=count.data_ptr() if append else 0, stream=stream)
        args = (n, d_ballots.data_ptr() if n else 0, 0 if d_status is None else d_status.data_ptr(), self.n_prior, board.data_ptr(), self.cap)
        if indexed:
            p.weed_indexed_device(*args, self.index.data_ptr(), self.index_seed, seed, scratch.data_ptr() if need else 0, dup.data_ptr(),
                                  found.data_ptr(), **common)
        else:
            p.weed_device(*args, seed, scratch.data_ptr() if need else 0, dup.data_ptr(), found.data_ptr(), **common)
        torch.cuda.synchronize()
        assert bytes(scratch[need:].cpu().numpy()) == bytes([CANARY]) * 64, "the pass wrote behind its scratch"
        assert dup[n:].cpu().tolist() == [0x5C5C5C5C] * 16, "the pass wrote behind dup_of"
        assert found[3].item() == 77
        assert bytes(board[self.cap * 64:].cpu().numpy()) == bytes([CANARY]) * 64, "the pass wrote behind the board"
        assert bytes(self.index[self.index_bytes:].cpu().numpy()) == bytes([CANARY]) * 64, "the pass wrote behind the index"
        return dict(dup=as_u32(dup[:n]), out=as_u32(out[:n]) if want_out else None, found=tuple(found[:3].cpu().tolist()), count=int(count.item()))

    def step(self, arr, status=None, append=True, alias=False, want_out=True, seed=0x1234567, stream=0, d_ballots=None):
        """one batch through both passes and the model; the chain's board, index and model move on if the append fitted -> the results"""
        torch, shape, n = self.torch, self.shape, len(arr)
        if d_ballots is None:
            d_ballots = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).cuda() if n else None
        dup, out, appended = W.weed(shape.keys(arr), status, self.model)
        fits = self.n_prior + len(appended) <= self.cap
        board_s, board_before, index_before = self.board.clone(), self.board.clone(), self.index.clone()
        stateless = self._pass(False, d_ballots, n, status, board_s, append, alias, want_out, seed ^ 0x55, stream)
        indexed = self._pass(True, d_ballots, n, status, self.board, append, alias, want_out, seed, stream)
        assert indexed == stateless, "the indexed pass differs from eg_*_weed_device over the same board"
        assert torch.equal(self.board, board_s), "the boards differ"
        assert indexed["dup"] == dup and (not want_out or indexed["out"] == out)
        assert indexed["found"] == W.found(dup) + (0 if fits or not append else 1,)
        if append and fits:
            assert indexed["count"] == self.n_prior + len(appended)
            assert bytes(self.board[64 * self.n_prior:64 * indexed["count"]].cpu().numpy()) == b"".join(appended)
            assert torch.equal(self.board[:64 * self.n_prior], board_before[:64 * self.n_prior])
            assert torch.equal(self.board[64 * indexed["count"]:], board_before[64 * indexed["count"]:])
            self.model += appended
        else:
            assert indexed["count"] == (self.n_prior if append else -5)
            assert torch.equal(self.board, board_before), "nothing was appended, yet the board changed"
            assert torch.equal(self.index, index_before), "nothing was appended, yet the index changed"
        return dict(indexed, model_dup=dup, model_out=out, appended=appended)

    def check_find_everything(self, extra_absent=50):
        """every board entry at its smallest position and absent keys nowhere, over the maintained index and over a freshly built one"""
        first = {}
        for j, key in enumerate(self.model):
            first.setdefault(key, j)
        queries = list(self.model) + random_keys(777, extra_absent)
        want = [first.get(q, NONE) for q in queries]
        assert self.find(queries) == want
        fresh_seed = self.index_seed ^ 0x1111
        assert self.find(queries, index=self.new_index(fresh_seed), seed=fresh_seed) == want


# ------------------------------------------------------------------ sizes and lanes
@pytest.mark.parametrize("n_start", [0, 1, 300])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_three_consecutive_batches_at_the_seams(torch, ctx, single5, n, n_start):
    """copies at lanes 0, 63, 64 and last - of the start board, of ballots appended one batch and two batches earlier, whole ballots and
    single keys at another option position - at the seams of wavefronts, blocks and (1025) the tiles of the scan over the keep flags"""
    start = random_keys(1000 + n_start, n_start)
    chain = Chain(torch, ctx, single5, start, n_start + 3 * n * 5)
    lanes = sorted({0, 63, 64, n - 1} & set(range(n)))
    earlier = []
    for t in range(3):
        arr = single5.random_ballots(7 * n + t, n)
        for i, at in enumerate(lanes):
            kinds = (["board"] if start else []) + (["prev1"] if t >= 1 else []) + (["prev2"] if t >= 2 else [])
            if not kinds:
                continue
            kind = kinds[(i + t) % len(kinds)]
            if kind == "board":
                arr[at, single5.key_slice((i + 3) % 5)] = np.frombuffer(start[(i * 97) % n_start], dtype=np.uint8)
            else:
                src = earlier[t - 1 if kind == "prev1" else t - 2]
                if i % 2:
                    arr[at, single5.key_slice(4)] = src[at, single5.key_slice(1)]
                else:
                    arr[at] = src[at]
        got = chain.step(arr)
        if t >= 1:
            assert got["dup"].count(PRIOR) >= 1
        if t == 0 and not start:
            assert got["dup"] == [NONE] * n and got["count"] == 5 * n
        assert got["found"][2] == 0
        earlier.append(arr)
    chain.check_find_everything()


def test_4096_identical_ballots_then_again(torch, ctx, single5):
    """every atomic of the batch table and of the index lands on five words; the second batch is on the board throughout"""
    arr = np.repeat(single5.random_ballots(1, 1), 4096, axis=0)
    chain = Chain(torch, ctx, single5, [], 4096 * 5)
    got = chain.step(arr)
    assert got["dup"] == [NONE] + [0] * 4095 and got["found"] == (0, 4095, 0) and got["out"] == [0] + [DUPLICATE] * 4095 and got["count"] == 5
    got = chain.step(arr, seed=99)
    assert got["dup"] == [PRIOR] * 4096 and got["found"] == (4096, 0, 0) and got["count"] == 5
    chain.check_find_everything()


# ------------------------------------------------------------------ find
def test_find(torch, ctx, single5):
    start = random_keys(31, 300)
    start[17], start[250], start[299] = start[3], start[3], start[0]          # equal bytes at several positions: the smallest
    chain = Chain(torch, ctx, single5, start, 300 + 2 * 65 * 5)
    absent = random_keys(32, 70)
    for n_q in (1, 64, 65):
        assert chain.find(start[:n_q]) == list(range(min(n_q, 17))) + [3 if j == 17 else j for j in range(17, n_q)]
        assert chain.find(absent[:n_q]) == [NONE] * n_q
    first = {}
    for j, key in enumerate(start):
        first.setdefault(key, j)
    assert chain.find(start + absent) == [first[k] for k in start] + [NONE] * 70
    assert chain.find([start[250], absent[0], start[299], start[17]]) == [3, NONE, 0, 3]
    assert chain.find([]) == []
    # two batches later: the maintained index against a fresh build over the final board; a ballot that carries a key twice is kept and
    # makes two equal board entries
    for t in range(2):
        arr = single5.random_ballots(900 + t, 65)
        arr[5, single5.key_slice(2)] = arr[5, single5.key_slice(0)]
        arr[64, single5.key_slice(1)] = np.frombuffer(start[299], dtype=np.uint8)
        got = chain.step(arr)
        assert got["dup"][5] == NONE and got["dup"][64] == PRIOR
    assert len(set(chain.model)) == len(chain.model) - 3 - 2
    chain.check_find_everything()
    assert chain.find(absent) == [NONE] * 70


# ------------------------------------------------------------------ append and read-only
def test_append_one_entry_short_changes_neither_board_nor_index(torch, ctx, single5):
    start = random_keys(41, 7)
    arr = single5.random_ballots(42, 300)
    arr[100] = arr[50]
    arr[200, single5.key_slice(0)] = np.frombuffer(start[6], dtype=np.uint8)
    status = [0 if b % 11 else 4 for b in range(300)]
    _, _, appended = W.weed(single5.keys(arr), status, start)
    fit = 7 + len(appended)
    short = Chain(torch, ctx, single5, start, fit - 1)
    got = short.step(arr, status=status)                       # step() compares board and index bytes before and after
    assert got["found"][2] == 1 and got["count"] == 7 and short.n_prior == 7
    short.check_find_everything()
    exact = Chain(torch, ctx, single5, start, fit)
    got = exact.step(arr, status=status)
    assert got["found"][2] == 0 and got["count"] == fit == exact.n_prior
    exact.check_find_everything()
    again = exact.step(arr, status=status)                     # the board is full: everything is on it, nothing more to append
    assert again["count"] == fit and again["dup"] == [PRIOR if s == 0 else NONE for s in status]


def test_the_read_only_form_leaves_the_index_alone(torch, ctx, single5):
    start = random_keys(51, 30)
    chain = Chain(torch, ctx, single5, start, 30 + 257 * 5)
    arr = single5.random_ballots(52, 257)
    arr[256, single5.key_slice(3)] = np.frombuffer(start[29], dtype=np.uint8)
    arr[64] = arr[63]
    got = chain.step(arr, append=False)                        # step() compares board and index bytes before and after
    assert got["dup"][256] == PRIOR and got["dup"][64] == 63 and got["count"] == -5 and chain.n_prior == 30
    three = [chain.step(arr, append=False, seed=s) for s in (0, 1, 0xFFFFFFFFFFFFFFFF)]
    assert three[0] == three[1] == three[2] == got
    empty = chain.step(arr[:0])
    assert empty["dup"] == [] and empty["found"] == (0, 0, 0) and empty["count"] == 30 and single5.p.weed_indexed_scratch_bytes(0) == 0


# ------------------------------------------------------------------ status words, streams, twice
def test_status_words_alias_stream_and_the_same_call_twice(torch, ctx, single5):
    arr = single5.random_ballots(5, 130)
    status = [0] * 130
    for b in (0, 9, 64, 100):
        status[b] = 6 + (b << 8)
    arr[10], arr[70], arr[64], arr[129], arr[101] = arr[9], arr[10], arr[3], arr[100], arr[4]
    start = random_keys(61, 12)
    base = Chain(torch, ctx, single5, start, 12 + 2 * 130 * 5)
    plain = base.step(arr, status=status, append=False)
    dup = plain["dup"]
    assert dup[10] == NONE and dup[70] == 10 and dup[64] == NONE and plain["out"][64] == 6 + (64 << 8) and dup[129] == NONE and dup[101] == 4
    assert base.step(arr, status=status, append=False, alias=True) == plain                   # status_out is d_status itself
    assert base.step(arr, status=status, append=False, want_out=False)["dup"] == dup
    s = torch.cuda.Stream()
    first = base.step(arr, status=status, stream=s.cuda_stream, alias=True)
    assert first["dup"] == dup and first["count"] == 12 + 5 * (130 - 4 - 2)
    # the same call again: everything it appended the first time is on the board now
    second = base.step(arr, status=status, stream=s.cuda_stream)
    assert second["dup"] == [NONE if st else PRIOR for st in status] and second["count"] == first["count"]
    assert second["out"] == [st if st else DUPLICATE for st in status]
    base.check_find_everything()


@pytest.mark.parametrize("kind,n_options,arg", [("multi", 16, 3), ("qv", 3, 4)])
def test_other_election_shapes(torch, eg, ctx, oracle, pk, kind, n_options, arg):
    shape = Shape(eg, ctx, oracle, pk, kind, n_options, arg)
    try:
        ballots, board = W.planted(31, 70, n_options, 4)
        chain = Chain(torch, ctx, shape, board, 4 + 2 * 70 * n_options)
        earlier = None
        for t in range(2):
            arr = shape.random_ballots(31 + t, 70)
            if t == 0:
                for b, keys in enumerate(ballots):
                    for k, key in enumerate(keys):
                        arr[b, shape.key_slice(k)] = np.frombuffer(key, dtype=np.uint8)
            else:
                arr[69] = earlier[50]
                arr[0, shape.key_slice(n_options - 1)] = earlier[51, shape.key_slice(0)]
                if kind == "qv":                              # a copied partial or credit ciphertext - 64 bytes that are no key - is no duplicate
                    key_bytes = {32 * r + i for r in shape.r_items for i in range(64)}
                    free = [o for o in range(0, shape.size - 63, 32) if not key_bytes & set(range(o, o + 64))]
                    arr[30, free[0]:free[0] + 64] = earlier[30, free[0]:free[0] + 64]
            got = chain.step(arr)
            if t == 0:
                assert got["dup"][3] == got["dup"][35] == got["dup"][36] == PRIOR and got["dup"][7] == 2
            else:
                assert got["dup"][69] == got["dup"][0] == PRIOR and got["dup"][30] == NONE
            earlier = arr
        chain.check_find_everything()
    finally:
        shape.p.close()


# ------------------------------------------------------------------ end to end
def test_end_to_end_two_batches_verify_weed_tally(torch, ctx, single5):
    """300 valid ballots of the GPU generator and 20 whole copies behind them, in two batches: everything verifies, the indexed pass
    flags exactly the copies - those of batch 1 against the board, those of batch 2 with their index - and the tally over the weeded
    status words is the verify entry's tally of the originals alone"""
    p, size = single5.p, single5.size
    d = torch.zeros(320 * size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(9090, 0, 300, d.data_ptr())
    p.ctx.synchronize()
    view = d.view(320, size)
    src = [(13 * i + 2) % 300 for i in range(20)]
    view[300:] = view[torch.tensor(src, device="cuda")]
    torch.cuda.synchronize()
    arr = view.cpu().numpy()
    ballots = arr.tobytes()
    status, tally_all = p.verify_batch(ballots)
    _, tally_300 = p.verify_batch(ballots[: 300 * size])
    p.tally_reset()
    assert status == [0] * 320 and tally_all != tally_300
    chain = Chain(torch, ctx, single5, [], 320 * 5)
    one = chain.step(arr[:200], status=status[:200])
    assert one["dup"] == [NONE] * 200 and one["count"] == 1000
    two = chain.step(arr[200:], status=status[200:])
    want = [NONE] * 100 + [PRIOR if s < 200 else s - 200 for s in src]
    assert two["dup"] == want and PRIOR in want and any(x < 100 for x in want) and two["count"] == 1500
    t1, c1 = p.tally_grouped(ballots[: 200 * size], one["out"], [0] * 200, 1)
    t2, c2 = p.tally_grouped(ballots[200 * size:], two["out"], [0] * 120, 1)
    assert c1 == [200] and c2 == [100]
    p.tally_reset()
    p.tally_add(t1)
    p.tally_add(t2)
    assert p.tally_encode() == tally_300
    p.tally_reset()


def test_cpp_voting_example_with_a_board_index(tmp_path):
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "voting.cpp"),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-ldl", "-o", str(exe)])
    out = subprocess.run([str(exe), "--replays", "3", "--board-index", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "with 3 replayed ballots: 102 of 103 ballots verified" in out.stdout
    assert "weeding dropped 3 ballots" in out.stdout and "the weeded totals equal those without the replays" in out.stdout
    assert "board index" in out.stdout
    plain = subprocess.run([str(exe), "--replays", "3", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    two_lines = lambda text: [line for line in text.splitlines() if line.startswith(("weeding dropped", "the weeded totals"))]
    assert two_lines(out.stdout) == two_lines(plain.stdout) and len(two_lines(plain.stdout)) == 2


# ------------------------------------------------------------------ a loose guard: the board must not be paid for in every batch
def test_the_indexed_pass_is_cheaper_than_the_stateless_pass_over_a_large_board(torch, ctx, single5):
    """a board of 2^22 random keys (268 MB) and a batch of 2^12 generated ballots: both passes warm in the same process, HIP events, the
    median of three after one warm-up round.  The stateless pass clears a table of 2^24 slots and re-inserts the board; the indexed pass
    does neither.  No ratio is asserted."""
    p, n, n_prior = single5.p, 1 << 12, 1 << 22
    cap = n_prior + n * 5
    d = torch.zeros(n * single5.size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(4242, 0, n, d.data_ptr())
    p.ctx.synchronize()
    board = torch.randint(0, 256, (cap * 64,), dtype=torch.uint8, device="cuda")
    index = torch.empty(ctx.weed_index_bytes(cap), dtype=torch.uint8, device="cuda")
    found = torch.zeros(3, dtype=torch.int32, device="cuda")
    ctx.weed_index_build_device(n_prior, board.data_ptr(), cap, INDEX_SEED, index.data_ptr(), found.data_ptr())
    torch.cuda.synchronize()
    assert found.cpu().tolist()[0] == 0
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    big = torch.empty(p.weed_scratch_bytes(n, n_prior), dtype=torch.uint8, device="cuda")
    small = torch.empty(p.weed_indexed_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    assert small.numel() < big.numel() // 100
    dup_s, dup_i = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    found_s, found_i = torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def rebuild():                               # untimed: every round of the indexed pass starts from an index over exactly [0, n_prior)
        ctx.weed_index_build_device(n_prior, board.data_ptr(), cap, INDEX_SEED, index.data_ptr(), found.data_ptr(), stream=stream)
        torch.cuda.synchronize()

    def timed(fn, prepare=None):
        ms = []
        for _ in range(4):                       # the first round warms up
            if prepare:
                prepare()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms[1:])

    # both append the same bytes to the same place behind the same n_prior entries, so every round sees the same board
    stateless_ms = timed(lambda: p.weed_device(n, d.data_ptr(), status.data_ptr(), n_prior, board.data_ptr(), cap, 77, big.data_ptr(),
                                               dup_s.data_ptr(), found_s.data_ptr(), d_board_count=count.data_ptr(), stream=stream))
    indexed_ms = timed(lambda: p.weed_indexed_device(n, d.data_ptr(), status.data_ptr(), n_prior, board.data_ptr(), cap, index.data_ptr(),
                                                     INDEX_SEED, 78, small.data_ptr(), dup_i.data_ptr(), found_i.data_ptr(),
                                                     d_board_count=count[1:].data_ptr(), stream=stream), prepare=rebuild)
    print(f"board 2^22, batch 2^12: indexed {indexed_ms:.3f} ms ({small.numel()} B of scratch), stateless {stateless_ms:.3f} ms ({big.numel()} B)")
    assert found_s.cpu().tolist() == [0, 0, 0] == found_i.cpu().tolist() and count.cpu().tolist() == [cap, cap]
    assert as_u32(dup_i) == as_u32(dup_s) == [NONE] * n
    assert indexed_ms < stateless_ms
