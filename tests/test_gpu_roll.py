"""The voter-roll pass (eg_roll_cast / eg_roll_check and their _device forms) on the GPU.  The pass reads key indices, status words and
the roll, so most cases are hand-made arrays, and every expected value comes from the model of the rule in tests/roll_ref.py.  The
end-to-end case runs the chain signatures -> verify -> weed -> roll -> weighted tally over ballots of the GPU generator: the result is
byte for byte the weighted tally of exactly the ballots the model keeps."""
import random
import statistics
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import roll_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
POLICIES = (R.ROLL_LAST, R.ROLL_FIRST)
SUPERSEDED, OFF_ROLL, NOT_CAST = (R.status_word(d) for d in (R.SUPERSEDED, R.OFF_ROLL, R.NOT_CAST))
CANARY = 0x5C
CANARY64 = 0x5C5C5C5C5C5C5C5C


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


def u32(torch, values, pad=0):
    a = np.full(len(values) + pad, 0x5C5C5C5C, dtype=np.uint32)
    a[: len(values)] = np.asarray(values, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32)).cuda()


def u64(torch, values, pad=0):
    a = np.full(len(values) + pad, CANARY64, dtype=np.uint64)
    a[: len(values)] = np.asarray(values, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).cuda()


def as_u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def as_u64(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def run_dev(torch, eg, ctx, policy, idx, roll, seq_base=0, status=None, groups=None, weights=None, alias=False, want_out=True, want_displaced=True,
            stream=0, check=False):
    """the device entries with buffers of their own and a canary behind every array the library writes -> dict"""
    vr = eg.VoterRoll(ctx, policy)
    n, n_keys, PAD = len(idx), len(roll), 8
    d_idx = u32(torch, idx, 1)
    d_status = None if status is None else u32(torch, status, PAD)
    d_roll = u64(torch, roll, PAD)
    d_groups = None if groups is None else u32(torch, groups, 1)
    d_weights = None if weights is None else u64(torch, weights, 1)
    by = u64(torch, [7] * n, PAD)
    out = d_status if alias else (u32(torch, [0x77] * n, PAD) if want_out else None)
    go = None if groups is None else u32(torch, [5] * n, PAD)
    wo = None if weights is None else u64(torch, [5] * n, PAD)
    found = u32(torch, [77, 77, 77], PAD)                                  # the library WRITES the three words
    ptr = lambda t: 0 if t is None else t.data_ptr()                      # noqa: E731
    if check:
        torch.cuda.synchronize()
        vr.check_device(n, d_idx.data_ptr(), seq_base, d_roll.data_ptr(), n_keys, by.data_ptr(), found.data_ptr(), ptr(d_status), ptr(d_groups),
                        ptr(d_weights), ptr(out), ptr(go), ptr(wo), stream)
        disp = count = scratch = None
    else:
        need = vr.cast_scratch_bytes(n, n_keys)
        scratch = torch.full((need + 64,), CANARY, dtype=torch.uint8, device="cuda")
        disp = u64(torch, [9] * (2 * n), PAD) if want_displaced else None
        count = u64(torch, [12345], PAD) if want_displaced else None
        torch.cuda.synchronize()
        vr.cast_device(n, d_idx.data_ptr(), seq_base, d_roll.data_ptr(), n_keys, by.data_ptr(), found.data_ptr(), scratch.data_ptr(), need, ptr(d_status),
                       ptr(d_groups), ptr(d_weights), ptr(out), ptr(go), ptr(wo), ptr(disp), ptr(count), stream)
    torch.cuda.synchronize()
    res = {"superseded_by": as_u64(by)[:n], "found": as_u32(found)[:3], "roll": as_u64(d_roll)[:n_keys],
           "status_out": as_u32(out)[:n] if out is not None else None, "groups_out": as_u32(go)[:n] if go is not None else None,
           "weights_out": as_u64(wo)[:n] if wo is not None else None}
    # the canaries: behind the roll, the scratch, the displaced entries and every output
    assert as_u64(d_roll)[n_keys:] == [CANARY64] * PAD and as_u64(by)[n:] == [CANARY64] * PAD and as_u32(found)[3:] == [0x5C5C5C5C] * PAD
    for t32 in (out, go):
        assert t32 is None or as_u32(t32)[n:] == [0x5C5C5C5C] * PAD
    assert wo is None or as_u64(wo)[n:] == [CANARY64] * PAD
    if not check:
        assert scratch[need:].cpu().tolist() == [CANARY] * 64
        if want_displaced:
            c = as_u64(count)
            assert c[1:] == [CANARY64] * PAD and c[0] <= n
            d = as_u64(disp)
            res["displaced"] = list(zip(d[0:2 * c[0]:2], d[1:2 * c[0]:2]))
            assert d[2 * c[0]:2 * n] == [9] * (2 * (n - c[0])) and d[2 * n:] == [CANARY64] * PAD          # byte for byte: nothing behind the count
    return res


def same(got, want, keys=("superseded_by", "status_out", "groups_out", "weights_out", "found", "displaced")):
    for k in keys:
        if k in want and k in got and got[k] is not None:
            assert got[k] == want[k], (k, [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:5])


# ------------------------------------------------------------------ seams of wavefronts, blocks and scan tiles
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1025])
def test_re_voting_pairs_at_the_seams(torch, eg, ctx, n, policy):
    """every voter once, then re-voting pairs at lanes 0 / 63 / 64 / last and across the block and the scan-tile seam; a second batch
    in which every voter votes again displaces all of them under LAST (ranks across the tile seam at 1025) and nobody under FIRST"""
    idx, used = list(range(n)), set()
    for a, b in ((0, n - 1), (63, 64), (255, 256), (1023, 1024), (62, 63)):
        if b < n and a != b and not {a, b} & used:
            idx[b] = idx[a]
            used |= {a, b}
    model = R.Roll(n + 3, policy)
    want = model.cast(idx, 10)
    got = run_dev(torch, eg, ctx, policy, idx, [0] * (n + 3), 10)
    same(got, want)
    assert got["roll"] == model.words() and got["found"][0] == len(used) // 2 and got["displaced"] == []
    again = idx[::-1]
    want2 = model.cast(again, 10 + n)
    got2 = run_dev(torch, eg, ctx, policy, again, got["roll"], 10 + n)
    same(got2, want2)
    assert got2["roll"] == model.words()
    assert len(got2["displaced"]) == (n - len(used) // 2 if policy == R.ROLL_LAST else 0)


@pytest.mark.parametrize("policy", POLICIES)
def test_4096_ballots_of_one_voter(torch, eg, ctx, policy):
    n, v = 4096, 3
    got = run_dev(torch, eg, ctx, policy, [v] * n, [0] * 5, 1000)
    winner = n - 1 if policy == R.ROLL_LAST else 0
    assert got["status_out"] == [0 if b == winner else SUPERSEDED for b in range(n)]
    assert got["superseded_by"] == [R.SEQ_NONE if b == winner else 1000 + winner for b in range(n)]
    assert got["found"] == [n - 1, 0, 0] and got["displaced"] == []
    assert got["roll"] == [R.word(1000 + winner, policy) if k == v else 0 for k in range(5)]


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("prior", ["empty", "partial", "full"])
@pytest.mark.parametrize("n_keys", [1, 2, 300])
def test_rosters_and_prior_rolls(torch, eg, ctx, n_keys, prior, policy):
    rng = random.Random(n_keys * 7 + len(prior) + policy)
    n, seq_base = 500, 2000
    idx = [rng.randrange(n_keys) for _ in range(n)]
    fill = {"empty": 0.0, "partial": 0.5, "full": 1.0}[prior]
    roll = [R.word(rng.choice((rng.randrange(0, 2000), rng.randrange(2500, 9000))), policy) if rng.random() < fill else 0 for _ in range(n_keys)]
    groups, weights = [rng.randrange(1 << 24) for _ in range(n_keys)], [rng.randrange(1 << 64) for _ in range(n_keys)]
    model = R.Roll(n_keys, policy, roll)
    want = model.cast(idx, seq_base, None, groups, weights)
    got = run_dev(torch, eg, ctx, policy, idx, roll, seq_base, None, groups, weights)
    same(got, want)
    assert got["roll"] == model.words()
    if prior == "empty":
        assert got["displaced"] == []
    if prior == "full" and n_keys == 300:
        assert 10 < len(got["displaced"]) < n_keys


@pytest.mark.parametrize("policy", POLICIES)
def test_batches_in_any_order_then_check_and_cast_twice(torch, eg, ctx, policy):
    rng = random.Random(31 + policy)
    n_keys = 60
    batches = [(base, [rng.randrange(n_keys) for _ in range(n)], [0 if rng.random() < 0.85 else 4 | b << 8 for b in range(n)])
               for base, n in ((0, 150), (150, 90), (240, 200))]
    model = R.Roll(n_keys, policy)
    for base, idx, st in batches:
        model.cast(idx, base, st)
    rolls = []
    for order in ((0, 1, 2), (2, 0, 1)):
        roll = [0] * n_keys
        for k in order:
            base, idx, st = batches[k]
            roll = run_dev(torch, eg, ctx, policy, idx, roll, base, st)["roll"]
        rolls.append(roll)
    assert rolls[0] == rolls[1] == model.words()
    kept = 0
    for base, idx, st in batches:
        want = model.check(idx, base, st)
        got = run_dev(torch, eg, ctx, policy, idx, rolls[0], base, st, check=True)
        same(got, want)
        assert got["roll"] == rolls[0]
        kept += sum(o == 0 and s == 0 for o, s in zip(got["status_out"], st))
        twice = run_dev(torch, eg, ctx, policy, idx, rolls[0], base, st)                  # cast again: nothing moves
        assert twice["roll"] == rolls[0] and twice["displaced"] == [] and twice["found"][1] == 0
        same(twice, want, keys=("superseded_by", "status_out"))
    assert kept == sum(w != 0 for w in rolls[0])                                          # one counted ballot per voter with any
    # a check against an empty roll: nothing was cast
    base, idx, st = batches[0]
    got = run_dev(torch, eg, ctx, policy, idx, [0] * n_keys, base, st, check=True)
    same(got, R.Roll(n_keys, policy).check(idx, base, st))
    assert got["found"] == [0, st.count(0), 0] and NOT_CAST in got["status_out"]


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("alias", [False, True])
def test_hand_made_status_words_and_off_roll_indices(torch, eg, ctx, policy, alias):
    """a rejected ballot claims nothing and its word is handed on, whatever its key_index says; off-roll indices on accepted ballots are
    counted and never used as an index"""
    n_keys, n = 10, 300
    rng = random.Random(9)
    idx = [rng.randrange(n_keys) for _ in range(n)]
    status = [0] * n
    for b in range(0, n, 7):
        status[b] = (1 + b % 15) | b << 8
        idx[b] = (n_keys, 0xFFFFFFFF, 0x7FFFFFFF, b % n_keys)[b % 4]           # poisoned: never read
    status[n - 1], idx[n - 1] = 6, 4                                           # the last ballot of voter 4 is rejected: it must not win
    off = {11: n_keys, 12: n_keys + 1, 13: 0xFFFFFFFF, 200: 1 << 31}
    for b, v in off.items():
        assert status[b] == 0
        idx[b] = v
    groups, weights = list(range(100, 100 + n_keys)), [1 << (6 * v) for v in range(n_keys)]
    model = R.Roll(n_keys, policy)
    want = model.cast(idx, 50, status, groups, weights)
    got = run_dev(torch, eg, ctx, policy, idx, [0] * n_keys, 50, status, groups, weights, alias=alias)
    same(got, want)
    assert got["roll"] == model.words() and got["found"][2] == len(off) and all(got["status_out"][b] == OFF_ROLL for b in off)
    assert all(got["status_out"][b] == status[b] and got["superseded_by"][b] == R.SEQ_NONE for b in range(0, n, 7))
    kept = [b for b in range(n) if status[b] == 0 and got["status_out"][b] == 0]
    assert len(kept) == n_keys and all(got["groups_out"][b] == groups[idx[b]] and got["weights_out"][b] == weights[idx[b]] for b in kept)
    assert all(got["groups_out"][b] == R.GROUP_NONE and got["weights_out"][b] == 0 for b in range(n) if b not in kept)
    if policy == R.ROLL_LAST:
        assert model.best[4][1] != 50 + n - 1
    chk = run_dev(torch, eg, ctx, policy, idx, got["roll"], 50, status, groups, weights, alias=alias, check=True)
    same(chk, model.check(idx, 50, status, groups, weights))


@pytest.mark.parametrize("policy", POLICIES)
def test_optional_outputs_may_be_null(torch, eg, ctx, policy):
    rng = random.Random(2)
    idx = [rng.randrange(40) for _ in range(700)]
    roll = [R.word(5, policy) if v % 3 == 0 else 0 for v in range(40)]
    model = R.Roll(40, policy, roll)
    want = model.cast(idx, 100)
    bare = run_dev(torch, eg, ctx, policy, idx, roll, 100, want_out=False, want_displaced=False)
    assert bare["status_out"] is None and bare["superseded_by"] == want["superseded_by"] and bare["roll"] == model.words() and bare["found"] == want["found"]
    only_groups = run_dev(torch, eg, ctx, policy, idx, roll, 100, groups=list(range(40)))
    assert only_groups["weights_out"] is None and only_groups["groups_out"] == model.check(idx, 100, None, list(range(40)))["groups_out"]
    assert only_groups["displaced"] == want["displaced"]
    bare_check = run_dev(torch, eg, ctx, policy, idx, model.words(), 100, want_out=False, check=True)
    assert bare_check["superseded_by"] == want["superseded_by"]


# ------------------------------------------------------------------ the entry forms
@pytest.mark.parametrize("policy", POLICIES)
def test_entry_forms_agree_on_a_caller_stream_and_twice(torch, eg, ctx, policy):
    rng = random.Random(77)
    n_keys = 90
    idx = [rng.randrange(n_keys + 2) for _ in range(900)]
    status = [0 if rng.random() < 0.9 else 3 for _ in idx]
    roll = [R.word(rng.randrange(5000), policy) if rng.random() < 0.4 else 0 for _ in range(n_keys)]
    groups, weights = [v % 4 for v in range(n_keys)], [v * v for v in range(n_keys)]
    model = R.Roll(n_keys, policy, roll)
    want = model.cast(idx, 1000, status, groups, weights)
    vr = eg.VoterRoll(ctx, policy)
    stream = torch.cuda.Stream()
    for _ in range(2):
        res, new_roll = vr.cast(idx, roll, 1000, status, groups, weights)
        assert new_roll == model.words() and res.displaced == want["displaced"] and res.found == want["found"]
        assert (res.superseded_by, res.status_out, res.groups_out, res.weights_out) == (want["superseded_by"], want["status_out"], want["groups_out"], want["weights_out"])
        got = run_dev(torch, eg, ctx, policy, idx, roll, 1000, status, groups, weights, stream=stream.cuda_stream)
        same(got, want)
        assert got["roll"] == new_roll
        chk = vr.check(idx, new_roll, 1000, status, groups, weights)
        verdicts = model.check(idx, 1000, status, groups, weights)
        assert (chk.superseded_by, chk.status_out, chk.groups_out, chk.weights_out, chk.found) == (
            verdicts["superseded_by"], verdicts["status_out"], verdicts["groups_out"], verdicts["weights_out"], verdicts["found"])
        assert res.kept(status) == chk.kept(status) == model.kept(idx, 1000, status)
    no_disp, _ = vr.cast(idx, roll, 1000, status, displaced=False)
    assert no_disp.displaced is None and no_disp.found == want["found"] and no_disp.groups_out is None


def test_n_zero(torch, eg, ctx):
    vr = eg.VoterRoll(ctx, R.ROLL_LAST)
    res, roll = vr.cast([], [5, 0, 9])
    assert roll == [5, 0, 9] and res.found == [0, 0, 0] and res.displaced == [] and res.status_out == []
    assert vr.check([], [5, 0, 9]).found == [0, 0, 0] and vr.cast([], [])[1] == []
    assert vr.cast_scratch_bytes(0, 3) == 0 and vr.cast_scratch_bytes(1, 1) == 768 and vr.cast_scratch_bytes(1025, 300) == 1280 + 4352 + 256
    d_roll, found, count = u64(torch, [5, 0, 9]), u32(torch, [7, 7, 7]), u64(torch, [99])
    torch.cuda.synchronize()
    vr.cast_device(0, 0, 0, d_roll.data_ptr(), 3, 0, found.data_ptr(), 0, 0, d_displaced=0, d_displaced_count=0)
    vr.cast_device(0, 0, 0, 0, 0, 0, 0, 0, 0)
    vr.check_device(0, 0, 0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert as_u64(d_roll) == [5, 0, 9] and as_u32(found) == [0, 0, 0]
    disp = u64(torch, [1, 1])
    vr.cast_device(0, 0, 0, d_roll.data_ptr(), 3, 0, found.data_ptr(), 0, 0, d_displaced=disp.data_ptr(), d_displaced_count=count.data_ptr())
    torch.cuda.synchronize()
    assert as_u64(count) == [0] and as_u64(disp) == [1, 1]


def test_every_refusal_with_a_live_context(torch, eg, ctx):
    vr = eg.VoterRoll(ctx, R.ROLL_LAST)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    base, top = buf.data_ptr(), (1 << 63) - 1
    torch.cuda.synchronize()

    def cast(n=1, idx=base, seq_base=0, roll=base, n_keys=1, by=base, found=base, scratch=base, sbytes=4096, policy=R.ROLL_LAST, **kw):
        eg.VoterRoll(ctx, policy).cast_device(n, idx, seq_base, roll, n_keys, by, found, scratch, sbytes, **kw)

    def check(n=1, idx=base, seq_base=0, roll=base, n_keys=1, by=base, found=base, policy=R.ROLL_LAST, scratch=0, sbytes=0, d_displaced=0,
              d_displaced_count=0, **kw):
        eg.VoterRoll(ctx, policy).check_device(n, idx, seq_base, roll, n_keys, by, found, **kw)

    for call in (cast, check):
        for kw, text in (({"n": 1 << 31}, "n is 2\\^31 or more"), ({"n_keys": 0}, "n_keys is 0"), ({"n_keys": (1 << 31) + 1}, "above EG_ROLL_KEYS_MAX"),
                         ({"seq_base": top}, "seq_base \\+ n is above"), ({"policy": 0}, "policy is neither"), ({"policy": 7}, "policy is neither"),
                         ({"idx": 0}, "null key_index"), ({"roll": 0}, "null key_index"), ({"by": 0}, "null key_index"), ({"found": 0}, "null key_index"),
                         ({"d_groups_out": base}, "groups_out without roster_groups"), ({"d_weights_out": base}, "weights_out without roster_weights"),
                         ({"roll": base + 4}, "8-byte aligned"), ({"by": base + 4}, "8-byte aligned"), ({"idx": base + 2}, "4-byte aligned"),
                         ({"d_status_in": base + 1}, "4-byte aligned"), ({"found": base + 1}, "4-byte aligned")):
            with pytest.raises(eg.EgError, match=text):
                call(**kw)
    for kw, text in (({"d_displaced": base}, "come together"), ({"d_displaced_count": base}, "come together"), ({"scratch": 0}, "scratch is null or too small"),
                     ({"sbytes": 767}, "scratch is null or too small"), ({"scratch": base + 2}, "4-byte aligned"),
                     ({"d_displaced": base + 4, "d_displaced_count": base}, "8-byte aligned")):
        with pytest.raises(eg.EgError, match=text):
            cast(**kw)
    with pytest.raises(eg.EgError, match="policy is neither"):
        eg.VoterRoll(ctx, 0).cast([0], [0])
    with pytest.raises(eg.EgError, match="n_keys is 0"):
        vr.check([0], [])
    torch.cuda.synchronize()
    assert int(buf.sum().item()) == 0                                          # nothing was launched
    assert vr.cast_scratch_bytes(1 << 31, 1) == 0 and vr.cast_scratch_bytes(1, 0) == 0 and vr.cast_scratch_bytes(1, (1 << 31) + 1) == 0


def test_passes_beside_a_verifying_thread(torch, eg, ctx, oracle):
    """two threads cast into rolls of their own while a third verifies ballots on the same context: the pass takes no lock"""
    pk = oracle.keypair_from_seed(12345)[1]
    p = eg.ChoiceParams(ctx, pk, 5, True)
    n = 2000
    d = torch.zeros(n * p.ballot_size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(808, 0, n, d.data_ptr())
    p.ctx.synchronize()
    rng = random.Random(6)
    idx = [rng.randrange(500) for _ in range(n)]
    wants = {}
    for k, policy in enumerate(POLICIES):
        model = R.Roll(500, policy)
        wants[k] = (model.cast(idx, 0), model.words())
    errors, results = [], {}

    def caster(k):
        try:
            s = torch.cuda.Stream()
            results[k] = [run_dev(torch, eg, ctx, POLICIES[k], idx, [0] * 500, stream=s.cuda_stream) for _ in range(3)]
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

    threads = [threading.Thread(target=caster, args=(0,)), threading.Thread(target=caster, args=(1,)), threading.Thread(target=verifier)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    p.tally_reset()
    assert not errors, errors
    assert results["status"] == [0] * n
    for k in (0, 1):
        for run in results[k]:
            same(run, wants[k][0])
            assert run["roll"] == wants[k][1]


@pytest.mark.parametrize("policy", POLICIES)
def test_large_batch_against_the_model_on_every_ballot(torch, eg, ctx, policy):
    """2^17 + 3 ballots with random indices over 50 000 keys above a half-filled roll: more than one iteration of the scan's top kernel"""
    n, n_keys = (1 << 17) + 3, 50_000
    rng = np.random.default_rng(17 + policy)
    idx = rng.integers(0, n_keys, n).tolist()
    status = (rng.random(n) < 0.05).astype(np.uint32).tolist()
    roll = [R.word(int(s), policy) if on else 0 for s, on in zip(rng.integers(0, 1 << 40, n_keys), rng.random(n_keys) < 0.5)]
    weights = rng.integers(0, 1 << 63, n_keys).tolist()
    model = R.Roll(n_keys, policy, roll)
    seq_base = 1 << 39
    want = model.cast(idx, seq_base, status, None, weights)
    got = run_dev(torch, eg, ctx, policy, idx, roll, seq_base, status, None, weights)
    same(got, want)
    assert got["roll"] == model.words() and len(got["displaced"]) > 64 * 64 // 8 and n > 64 * 1024


@pytest.mark.parametrize("policy", POLICIES)
def test_rolls_of_two_slabs_merge_by_the_maximum(torch, eg, ctx, policy):
    rng = random.Random(4 + policy)
    n_keys, n = 200, 1500
    idx = [rng.randrange(n_keys) for _ in range(n)]
    status = [0 if rng.random() < 0.9 else 2 for _ in range(n)]
    cut = 700
    a = run_dev(torch, eg, ctx, policy, idx[:cut], [0] * n_keys, 0, status[:cut])["roll"]
    b = run_dev(torch, eg, ctx, policy, idx[cut:], [0] * n_keys, cut, status[cut:])["roll"]
    merged = as_u64(torch.maximum(u64(torch, a), u64(torch, b)))
    whole = run_dev(torch, eg, ctx, policy, idx, [0] * n_keys, 0, status)
    model = R.Roll(n_keys, policy)
    model.cast(idx, 0, status)
    assert merged == whole["roll"] == model.words() == R.merge(a, b)
    first = run_dev(torch, eg, ctx, policy, idx[:cut], merged, 0, status[:cut], check=True)
    second = run_dev(torch, eg, ctx, policy, idx[cut:], merged, cut, status[cut:], check=True)
    assert first["status_out"] + second["status_out"] == whole["status_out"] == model.check(idx, 0, status)["status_out"]
    assert first["superseded_by"] + second["superseded_by"] == whole["superseded_by"]
    from elastic_elgamal_amd import distributed as egd
    t = u64(torch, a)
    assert egd.merge_rolls(t) is t


# ------------------------------------------------------------------ end to end
def test_end_to_end_signatures_verify_weed_roll_weighted_tally(torch, eg, ctx, oracle):
    """300 generated five-option ballots plus 20 re-votes with another choice (one of them with a broken signature: it must not claim its
    voter's slot): sign, the signature pass, verify, weed, roll, tally_weighted over status_out, groups_out, weights_out.  Byte for byte
    the weighted tally of exactly the ballots the model keeps; under FIRST that of the first ballots."""
    pk = oracle.keypair_from_seed(12345)[1]
    p = eg.ChoiceParams(ctx, pk, 5, True)
    ed = eg.Ed25519(ctx)
    size, voters, revoters = p.ballot_size, 300, [(13 * i + 2) % 300 for i in range(20)]
    choice = [v % 5 for v in range(voters)]
    selections = [1 << choice[v] for v in range(voters)] + [1 << ((choice[v] + 1) % 5) for v in revoters]
    ballots = p.encrypt_selected(777, 0, selections)
    n = len(selections)
    key_index = list(range(voters)) + revoters
    seeds = [bytes([v % 251, v // 251]) * 16 for v in range(voters)]
    keys = ed.keypairs(b"".join(seeds))
    sigs = bytearray(ed.sign(b"".join(seeds[v] for v in key_index), ballots, size, b"election-18"))
    sigs[64 * 300 + 5] ^= 1                                        # the re-vote of voter `revoters[0]` is not signed by them
    st_sig = ed.verify(ballots, size, keys, bytes(sigs), b"election-18", key_index)
    assert [b for b, s in enumerate(st_sig) if s] == [300]
    st_verify, _ = p.verify_batch(ballots)
    p.tally_reset()
    assert st_verify == [0] * n
    status = [a or b for a, b in zip(st_sig, st_verify)]
    _, weeded, _ = p.weed(ballots, status)
    assert weeded == status                                        # fresh ciphertexts: a re-vote is no replay
    groups, weights = [v % 3 for v in range(voters)], [1 + v % 7 for v in range(voters)]
    everything, _, _ = p.tally_weighted(ballots, weeded, [weights[v] for v in key_index], [groups[v] for v in key_index], 3, weight_bits=3)

    def tally_of(kept):
        picked = b"".join(ballots[b * size:(b + 1) * size] for b in kept)
        return p.tally_weighted(picked, [0] * len(kept), [weights[key_index[b]] for b in kept], [groups[key_index[b]] for b in kept], 3, weight_bits=3)

    for policy in POLICIES:
        model = R.Roll(voters, policy)
        want = model.cast(key_index, 0, weeded, groups, weights)
        kept = [b for b in range(n) if want["status_out"][b] == 0]
        res, roll = eg.VoterRoll(ctx, policy).cast(key_index, [0] * voters, 0, weeded, groups, weights)
        assert res.status_out == want["status_out"] and res.groups_out == want["groups_out"] and res.weights_out == want["weights_out"]
        assert roll == model.words() and res.found == [19, 0, 0] and len(kept) == voters
        tallies, sums, counts = p.tally_weighted(ballots, res.status_out, res.weights_out, res.groups_out, 3, weight_bits=3)
        assert (tallies, sums, counts) == tally_of(kept) and tallies != everything and sum(counts) == voters
        if policy == R.ROLL_FIRST:
            assert kept == list(range(voters)) and (tallies, sums, counts) == tally_of(range(voters))
        else:
            assert kept == [b for b in range(voters) if b not in revoters[1:]] + list(range(301, n))
            assert res.superseded_by[revoters[1]] == 301 and res.superseded_by[revoters[0]] == R.SEQ_NONE and res.status_out[300] == st_sig[300]


def test_cpp_voting_example_with_revotes(tmp_path):
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "voting.cpp"),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    out = subprocess.run([str(exe), "--revotes", "5", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "with 5 re-votes: 104 of 105 ballots verified" in out.stdout and "the roll superseded 5 ballots" in out.stdout
    assert "ballot #1 superseded by ballot #101" in out.stdout and "the totals equal those of the last ballots" in out.stdout
    assert "OK: the decrypted totals equal the expected ones" in out.stdout
    for flags in (["--precincts", "4"], ["--weighted"], ["--precincts", "3", "--weighted"]):
        out = subprocess.run([str(exe), *flags, "--revotes", "5", "100", "5", "7"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "the roll superseded 5 ballots" in out.stdout and "OK: the decrypted totals equal the expected ones" in out.stdout


# ------------------------------------------------------------------ a loose guard against a pass that has gone serial
def test_flooding_one_key_is_cheaper_than_checking_the_signatures(torch, eg, ctx):
    """at 2^16 items the flood case of cast_device (every ballot under one key: every atomic of the batch on one address) takes less time
    than eg_ed25519_verify_device over 2^16 32-byte messages in the same process (warm, median of three, HIP events).  The signature
    pass does a 252-doubling chain per item."""
    n, n_keys = 1 << 16, 1 << 16
    ed, vr = eg.Ed25519(ctx), eg.VoterRoll(ctx, R.ROLL_LAST)
    seeds = torch.from_numpy(np.random.default_rng(1).integers(0, 256, n * 32, dtype=np.uint8)).cuda()
    msgs = torch.from_numpy(np.random.default_rng(2).integers(0, 256, n * 32, dtype=np.uint8)).cuda()
    keys, sigs = torch.zeros(n * 32, dtype=torch.uint8, device="cuda"), torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    ed.keypairs_device(n, seeds.data_ptr(), keys.data_ptr())
    ed.sign_device(n, seeds.data_ptr(), msgs.data_ptr(), 32, 32, sigs.data_ptr())
    st = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    ed_need = ed.verify_scratch_bytes(n)
    ed_scratch = torch.empty(ed_need, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")                  # the flood: every ballot under key 0
    roll, by = torch.zeros(n_keys, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    out, found = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    disp, count = torch.zeros(2 * n, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    need = vr.cast_scratch_bytes(n, n_keys)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

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

    stream = torch.cuda.current_stream().cuda_stream
    sig_ms = timed(lambda: ed.verify_device(n, msgs.data_ptr(), 32, 32, keys.data_ptr(), n, sigs.data_ptr(), st.data_ptr(), ed_scratch.data_ptr(), ed_need,
                                            stream=stream))

    def flood():
        roll.zero_()
        vr.cast_device(n, idx.data_ptr(), 0, roll.data_ptr(), n_keys, by.data_ptr(), found.data_ptr(), scratch.data_ptr(), need, d_status_out=out.data_ptr(),
                       d_displaced=disp.data_ptr(), d_displaced_count=count.data_ptr(), stream=stream)

    flood_ms = timed(flood)
    print(f"n = 2^16: flood cast {flood_ms:.3f} ms, signature pass {sig_ms:.3f} ms")
    assert int(st.abs().sum().item()) == 0                                  # every signature holds
    assert as_u32(found) == [n - 1, 0, 0] and int(roll[0].item()) == n and int(roll[1:].abs().sum().item()) == 0 and int(count.item()) == 0
    assert flood_ms < sig_ms
