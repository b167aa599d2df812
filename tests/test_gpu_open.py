"""The ballot-audit pass (eg_*_open_check[_device]) and the opener (eg_*_open_batch[_device]) on the GPU.  Ballots come from the GPU
generators, openings from the opener; every expected status word comes from the model tests/open_ref.py over the oracle's primitives, and
the opener itself is judged by that model, not by the checker."""
import numpy as np
import pytest

import open_cases as K
import open_ref as R

pytestmark = pytest.mark.gpu

L = R.L
CANARY = 0x5C


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


@pytest.fixture(scope="module")
def group(oracle, pk):
    return R.oracle_group(oracle, pk)


_PARAMS = {}


def params(eg, ctx, oracle, pk, kind, no, arg=0):
    """(params object, slot offsets), one per shape for the module"""
    key = (kind, no, arg)
    if key not in _PARAMS:
        if kind == "qv":
            _PARAMS[key] = (eg.QuadraticVotingParams(ctx, pk, no, arg), R.qv_slots(no, oracle.QvParams(pk, no, arg).vote_size))
        else:
            _PARAMS[key] = (eg.ChoiceParams(ctx, pk, no, kind == "single"), R.choice_slots(no))
    return _PARAMS[key]


def selections(kind, no, n, k=3):
    if kind == "single":
        return [1 << ((7 * i + 3) % no) for i in range(n)]
    return [sum(1 << ((i + 5 * j) % no) for j in range(k)) for i in range(n)]


def make(p, kind, no, seed, first, n, skip, given=True, arg=0, torch=None):
    """(ballots, values, rand) from the generator and the opener with the same arguments"""
    if kind == "qv":
        if given:
            top = int(arg ** 0.5)
            votes = [[(top if k == i % no and i % 3 == 0 else (i + k) % 2 if (i % 3 == 1 and k < 2) else 0) for k in range(no)] for i in range(n)]
            assert all(sum(v * v for v in vs) <= arg for vs in votes)
            return (p.encrypt_votes(seed, first, votes, skip),) + p.open_batch(seed, first, n, votes, skip)
        buf = torch.zeros(max(n * p.ballot_size, 1), dtype=torch.uint8, device="cuda")
        p.encrypt_batch_device(seed, first, n, buf.data_ptr())
        torch.cuda.synchronize()
        return (buf.cpu().numpy().tobytes()[: n * p.ballot_size],) + p.open_batch(seed, first, n)
    if given:
        sel = selections(kind, no, n)
        return (p.encrypt_selected(seed, first, sel, skip),) + p.open_batch(seed, first, n, sel, skip)
    return (p.encrypt_batch(seed, first, n, arg),) + p.open_batch(seed, first, n, None, 0, arg)


def split(p, slots, ballots, values, rand):
    no, size = len(slots), p.ballot_size
    n = len(ballots) // size
    return [K.Opened(ballots[b * size:(b + 1) * size], values[b * no:(b + 1) * no], [rand[32 * (b * no + t):32 * (b * no + t + 1)] for t in range(no)])
            for b in range(n)]


def check_dev(torch, p, n, ballots, values, rand, status_in=None, alias=False):
    """the device entry with buffers of its own and a canary behind the scratch and the status words -> (status_out, found)"""
    d_b = torch.frombuffer(bytearray(ballots or b"\0"), dtype=torch.uint8).cuda()
    d_v = torch.from_numpy(np.asarray(values or [0], dtype=np.uint64).view(np.int64).copy()).cuda()
    d_r = torch.frombuffer(bytearray(rand or b"\0"), dtype=torch.uint8).cuda()
    need = p.open_check_scratch_bytes(n)
    assert need == (4 * n * p.n_options + 255) // 256 * 256
    scratch = torch.full((need + 64,), CANARY, dtype=torch.uint8, device="cuda")
    d_in = None if status_in is None else torch.from_numpy(np.asarray(status_in, dtype=np.uint32).view(np.int32).copy()).cuda()
    out = torch.full((n + 16,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
    if alias:
        out[:n] = d_in
    found = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p.open_check_device(n, d_b.data_ptr(), d_v.data_ptr(), d_r.data_ptr(), out.data_ptr(), found.data_ptr(), scratch.data_ptr(),
                        d_status_in=(out.data_ptr() if alias else d_in.data_ptr()) if d_in is not None else 0)
    torch.cuda.synchronize()
    assert bool((scratch[need:] == CANARY).all()) and bool((out[n:] == 0x5C5C5C5C).all())
    return [v & 0xFFFFFFFF for v in out[:n].cpu().tolist()], found.cpu().tolist()


# ------------------------------------------------------------------ accept path
ACCEPT = [  # (kind, n_options, arg, n, rng_skip, first, given)
    ("single", 1, 0, 63, 0, 0, True), ("single", 2, 0, 64, 1, 3, True), ("single", 5, 0, 1, 5, 9, True), ("single", 5, 0, 65, 0, 1, True),
    ("single", 5, 0, 257, 1, 0, True), ("single", 5, 0, 1000, 5, 77, True), ("single", 5, 0, 1000, 0, 5, False), ("single", 31, 0, 65, 1, 2, True),
    ("single", 32, 0, 64, 5, 1, True), ("single", 33, 0, 63, 0, 4, True), ("single", 33, 0, 65, 0, 4, False), ("single", 40, 0, 257, 1, 6, True),
    ("multi", 16, 3, 257, 5, 8, True), ("multi", 16, 3, 64, 0, 2, False), ("qv", 2, 7, 1000, 1, 3, True), ("qv", 2, 7, 65, 0, 1, False),
    ("qv", 5, 20, 257, 5, 2, True), ("qv", 5, 20, 63, 0, 7, False),
]


@pytest.mark.parametrize("kind,no,arg,n,skip,first,given", ACCEPT)
def test_true_openings_are_accepted_and_the_ballots_verify(eg, torch, ctx, oracle, pk, kind, no, arg, n, skip, first, given):
    p, slots = params(eg, ctx, oracle, pk, kind, no, arg)
    ballots, values, rand = make(p, kind, no, 4200 + no, first, n, skip, given, arg, torch)
    status, found = p.open_check(ballots, values, rand)
    assert status == [0] * n and found == [n, 0]
    assert check_dev(torch, p, n, ballots, values, rand) == (status, found)
    assert p.verify_batch(ballots)[0] == [0] * n
    if kind != "qv":
        assert all(v in (0, 1) for v in values) and sum(values) == n * (1 if kind == "single" else arg)


def test_empty_pile(eg, torch, ctx, oracle, pk):
    p, _ = params(eg, ctx, oracle, pk, "single", 5)
    assert p.open_check(b"", [], b"") == ([], [0, 0]) and p.open_check_scratch_bytes(0) == 0
    assert p.open_batch(1, 0, 0) == ([], b"")
    found = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    p.open_check_device(0, 0, 0, 0, 0, found.data_ptr(), 0)
    torch.cuda.synchronize()
    assert found.cpu().tolist() == [0, 0]
    with pytest.raises(eg.EgError, match="EG_OPEN_ITEMS_MAX"):
        p.open_check_device((1 << 31) - 1, 256, 256, 256, 256, 256, 256)


# ------------------------------------------------------------------ the opener, judged by the model
@pytest.mark.parametrize("kind,no,arg,skip,given", [("single", 5, 0, 1, True), ("single", 33, 0, 0, False), ("multi", 16, 3, 5, True),
                                                     ("multi", 16, 3, 0, False), ("qv", 2, 7, 5, True), ("qv", 5, 20, 0, False), ("qv", 5, 20, 1, True)])
def test_the_opener_s_values_and_randomness_re_encrypt_to_the_wire_bytes(eg, torch, ctx, oracle, pk, group, kind, no, arg, skip, given):
    p, slots = params(eg, ctx, oracle, pk, kind, no, arg)
    n = 200
    ballots, values, rand = make(p, kind, no, 99 + no, 11, n, skip, given, arg, torch)
    cases = split(p, slots, ballots, values, rand)
    assert K.model(group, cases, slots) == ([0] * n, [n, 0])
    assert len({c.rands[0] for c in cases}) == n                     # every ballot has randomness of its own
    if kind == "qv" and not given:
        assert any(v for v in values)                                 # the second stream casts some votes


# ------------------------------------------------------------------ reject path
@pytest.fixture(scope="module")
def forged(eg, torch, ctx, oracle, pk, group):
    """1 000 single-choice ballots of five options, a tenth of them with one forgery: (params, slots, cases, the model's words)"""
    p, slots = params(eg, ctx, oracle, pk, "single", 5)
    n = 1000
    cases = split(p, slots, *make(p, "single", 5, 777, 4, n, 1))
    lanes = [0, 63, 64, n - 1] + [b for b in range(10, n, 10)][: n // 10 - 4]
    for j, b in enumerate(lanes):
        if j % 9 == 8:
            K.forge_other_opening(cases[b], cases[(b + 1) % n].copy())
        else:
            K.FORGERIES[j % 9](cases[b], (j // 9) % 5, slots)
    K.forge_v_plus_1(cases[64], 4, slots)                              # a second failure in a higher slot changes nothing
    want, found = K.model(group, cases, slots)
    assert found == [n, len(lanes)] and all(want[b] for b in lanes) and len({w for w in want}) > 12
    return p, slots, cases, lanes, want, found


def test_forgeries_get_the_model_s_status_words_on_both_forms(torch, forged):
    p, slots, cases, lanes, want, found = forged
    ballots, values, rand = K.flat(cases)
    assert p.open_check(ballots, values, rand) == (want, found)
    assert check_dev(torch, p, len(cases), ballots, values, rand) == (want, found)


def test_status_words_of_a_verify_call_are_handed_on(eg, torch, ctx, oracle, pk, group):
    p, slots = params(eg, ctx, oracle, pk, "single", 5)
    cases = split(p, slots, *make(p, "single", 5, 778, 2, 257, 1))
    for j, b in enumerate((5, 7, 65, 130, 200)):                       # forged openings of valid ballots; 5 and 130 will not participate
        K.FORGERIES[j](cases[b], j, slots)
    tampered = bytearray(K.flat(cases)[0])
    for b in (0, 5, 63, 64, 256):                                      # a flipped bit in a response, in a ciphertext, a non-canonical scalar
        tampered[b * p.ballot_size + (330 if b % 2 else 40)] ^= 0x04
    tampered[130 * p.ballot_size + 320:130 * p.ballot_size + 352] = b"\xff" * 32
    ballots = bytes(tampered)
    status_in = p.verify_batch(ballots)[0]
    assert status_in == oracle.ChoiceParams(pk, 5, True).verify_batch(ballots) and sum(1 for s in status_in if s) == 6
    for c, b in zip(cases, range(len(cases))):
        c.ballot = ballots[b * p.ballot_size:(b + 1) * p.ballot_size]
    want, found = K.model(group, cases, slots, status_in)
    assert all(want[b] == status_in[b] for b in (0, 5, 63, 64, 130, 256)) and found == [251, 3]
    assert [R.detail(want[b]) for b in (7, 65, 200)] == [(1, R.OPEN_B), (2, R.OPEN_B), (4, R.OPEN_BAD_SCALAR)]
    _, values, rand = K.flat(cases)
    poisoned_v, poisoned_r = list(values), bytearray(rand)
    for b in (0, 5, 63, 64, 130, 256):                                 # nothing of a ballot that does not participate is looked at
        poisoned_v[5 * b:5 * b + 5] = [0xEEEEEEEEEEEEEEEE] * 5
        poisoned_r[160 * b:160 * b + 160] = b"\xee" * 160
    assert p.open_check(ballots, poisoned_v, bytes(poisoned_r), status_in) == (want, found)
    for alias in (False, True):
        assert check_dev(torch, p, len(cases), ballots, poisoned_v, bytes(poisoned_r), status_in, alias) == (want, found)


def test_qv_forgeries(eg, torch, ctx, oracle, pk, group):
    p, slots = params(eg, ctx, oracle, pk, "qv", 5, 20)
    n = 65
    cases = split(p, slots, *make(p, "qv", 5, 31, 2, n, 1, True, 20))
    for j, b in enumerate((0, 7, 31, 63, 64)):
        K.FORGERIES[(3 * j + 1) % 8](cases[b], j % 5, slots)
    want, found = K.model(group, cases, slots)
    assert found == [n, 5]
    ballots, values, rand = K.flat(cases)
    assert p.open_check(ballots, values, rand) == (want, found) == check_dev(torch, p, n, ballots, values, rand)


# ------------------------------------------------------------------ the chain: audited ballots are spoiled
def test_audited_ballots_go_onto_the_board_and_a_recast_copy_is_flagged(eg, ctx, oracle, pk):
    p, slots = params(eg, ctx, oracle, pk, "single", 5)
    size = p.ballot_size
    audited, values, rand = make(p, "single", 5, 555, 0, 8, 0)
    values[7] ^= 1                                                      # one audit fails: its ballot is spoiled all the same
    status, found = p.open_check(audited, values, rand)
    assert found == [8, 1] and eg.status_kind(status[1]) == eg.ST_BAD_OPENING
    _, _, board = p.weed(audited, None, b"", append=True)               # the keys of EVERY audited ballot, whatever its verdict
    assert len(board) == 8 * 5 * 64
    cast = p.encrypt_selected(556, 100, selections("single", 5, 64), 0)
    recast = bytearray(cast)
    recast[3 * size:4 * size] = audited[2 * size:3 * size]              # a device re-casts a ballot it has opened
    recast = bytes(recast)
    st, tally = p.verify_batch(recast)
    assert st == [0] * 64
    dup, st_out, _ = p.weed(recast, st, board)
    assert dup == [eg.DUP_NONE] * 3 + [eg.DUP_PRIOR] + [eg.DUP_NONE] * 60 and st_out[3] == eg.ST_DUPLICATE
    tallies, counts = p.tally_grouped(recast, st_out, [0] * 64, 1)
    kept = cast[:3 * size] + cast[4 * size:]
    assert counts == [63] and tallies == p.verify_batch(kept)[1]        # the untouched ballots tally as before
