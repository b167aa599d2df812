"""The weighted per-group tally (eg_*_tally_weighted[_device]) on the GPU: ballots from the GPU generators, verdicts from the batch
entry, every group and slot against the CPU oracle's weighted sum (oracle.point_multi_mul over the wire items, tests/
weighted_tally_cases.py) - never against the code under test, except where the issue asks for identity with the grouped entry (all
weights 1) and for linearity at a size the oracle is too slow for."""
import random
import re
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import edge_ballots as E
import group_tally_cases as G
import weighted_tally_cases as W

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NONE = G.GROUP_NONE
S1, S2 = G.piece_sizes()
M64 = W.M64


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
    def __init__(self, eg, ctx, oracle, pk, kind, n_options, arg=0):
        self.kind, self.n_options, self.arg = kind, n_options, arg
        if kind == "qv":
            self.op = oracle.QvParams(pk, n_options, arg)
            self.p = eg.QuadraticVotingParams(ctx, pk, n_options, arg)
        else:
            self.op = oracle.ChoiceParams(pk, n_options, kind == "single")
            self.p = eg.ChoiceParams(ctx, pk, n_options, kind == "single")
        self.size = self.p.ballot_size
        assert self.size == self.op.ballot_size

    def generate(self, torch, seed, n):
        out = torch.zeros(max(n, 1) * self.size, dtype=torch.uint8, device="cuda")
        if self.kind == "qv":
            self.p.encrypt_batch_device(seed, 0, n, out.data_ptr())
        else:
            self.p.encrypt_batch_device(seed, 0, n, out.data_ptr(), n_selected=self.arg)
        self.p.ctx.synchronize()
        return out[: n * self.size]


@pytest.fixture(scope="module")
def single5(eg, ctx, oracle, pk):
    return Shape(eg, ctx, oracle, pk, "single", 5)


def u32(torch, values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def u64(torch, values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint64).view(np.int64).copy()).cuda()


def run_device(torch, shape, d_ballots, d_status, weights, bits, groups, n_groups, stream=0, with_sums=True):
    """the device entry with buffers of its own -> (tallies tensor [n_groups, 64 n_options], weight sums as ints, counts, bad tuple);
    a 4 KiB canary behind the scratch must come back untouched.  groups None: the NULL-groups form."""
    p, n = shape.p, len(weights)
    d_weights = u64(torch, weights) if n else None
    d_groups = u32(torch, groups) if groups is not None and n else None
    need = p.tally_weighted_scratch_bytes(n, n_groups)
    scratch = torch.full((need + 4096,), 0x5C, dtype=torch.uint8, device="cuda")
    tallies = torch.full((n_groups, 64 * shape.n_options), 0xAB, dtype=torch.uint8, device="cuda")
    sums = torch.full((n_groups, 2), -1, dtype=torch.int64, device="cuda")
    counts = torch.full((n_groups,), -1, dtype=torch.int32, device="cuda")
    bad = torch.full((3,), 77, dtype=torch.int32, device="cuda")          # the library WRITES all three words
    torch.cuda.synchronize()
    dummy = scratch.data_ptr()                                            # a non-NULL groups pointer for n == 0 with several groups
    p.tally_weighted_device(n, d_ballots.data_ptr() if n else 0, d_status.data_ptr() if n else 0, d_weights.data_ptr() if n else 0, bits,
                            d_groups.data_ptr() if d_groups is not None else (dummy if groups is not None else 0), n_groups,
                            scratch.data_ptr(), tallies.data_ptr(), bad.data_ptr(), d_weight_sums=sums.data_ptr() if with_sums else 0,
                            d_counts=counts.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert bool((scratch[need:] == 0x5C).all().item()), "the pass wrote behind its scratch"
    words = sums.cpu().numpy().view(np.uint64).tolist()
    return tallies, [lo | (hi << 64) for lo, hi in words], counts.cpu().tolist(), tuple(bad.cpu().tolist())


def run_grouped(torch, shape, d_ballots, d_status, groups, n_groups):
    p, n = shape.p, len(groups)
    scratch = torch.empty(max(p.tally_grouped_scratch_bytes(n, n_groups), 16), dtype=torch.uint8, device="cuda")
    tallies = torch.full((n_groups, 64 * shape.n_options), 0xCD, dtype=torch.uint8, device="cuda")
    counts = torch.full((n_groups,), -1, dtype=torch.int32, device="cuda")
    bad = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    p.tally_grouped_device(n, d_ballots.data_ptr(), d_status.data_ptr(), u32(torch, groups).data_ptr(), n_groups, scratch.data_ptr(),
                           tallies.data_ptr(), bad.data_ptr(), d_counts=counts.data_ptr())
    torch.cuda.synchronize()
    return tallies, counts.cpu().tolist(), tuple(bad.cpu().tolist())


def tamper(torch, d_ballots, size, which, seed):
    rng = random.Random(seed)
    view = d_ballots.view(-1, size)
    for b in which:
        view[b, 32 * rng.randrange(size // 32) + rng.randrange(32)] ^= 1 << rng.randrange(8)
    torch.cuda.synchronize()


def verified(torch, shape, seed, n, tampered=()):
    """n generated ballots, some tampered, and the batch entry's verdicts: (device ballots, bytes, status list, device status)"""
    d = shape.generate(torch, seed, n)
    tamper(torch, d, shape.size, tampered, seed + 1)
    ballots = bytes(d.cpu().numpy())
    status, _ = shape.p.verify_batch(ballots, with_tally=False)
    return d, ballots, status, u32(torch, status)


@pytest.fixture(scope="module")
def basic(torch, single5):
    """3 000 five-option ballots, a tenth tampered, verified by the batch entry; 7 groups of which group 3 is empty, 50 ballots in none"""
    n, n_groups = 3000, 7
    d, ballots, status, d_status = verified(torch, single5, 1501, n, range(3, n, 10))
    assert 2500 < status.count(0) <= 2700
    rng = random.Random(78)
    groups = [rng.choice((0, 1, 2, 4, 5, 6)) for _ in range(n)]
    for b in rng.sample(range(n), 50):
        groups[b] = NONE
    return dict(n=n, n_groups=n_groups, d=d, ballots=ballots, status=status, d_status=d_status, groups=groups)


# ------------------------------------------------------------------ 1. all weights 1
@pytest.mark.parametrize("bits", [1, 64])
def test_all_weights_one_is_the_grouped_tally_byte_for_byte(torch, single5, basic, bits):
    B = basic
    want, want_counts, bad = run_grouped(torch, single5, B["d"], B["d_status"], B["groups"], B["n_groups"])
    assert bad == (0, 0)
    tallies, sums, counts, bad = run_device(torch, single5, B["d"], B["d_status"], [1] * B["n"], bits, B["groups"], B["n_groups"])
    assert bad == (0, 0, 0) and counts == want_counts and sums == counts and counts[3] == 0
    assert torch.equal(tallies, want)
    assert single5.p.tally_weighted(B["ballots"], B["status"], [1] * B["n"], B["groups"], B["n_groups"], weight_bits=bits) == \
        (bytes(want.cpu().numpy()), counts, counts)


# ------------------------------------------------------------------ 2. random 64-bit weights
def test_random_64_bit_weights_against_the_oracle(torch, oracle, single5, basic):
    """600 ballots in 6 groups, weight_bits 64, the corner weights among random ones: every group and slot is the oracle's weighted sum;
    the weight sums are exact 128-bit numbers with a non-zero high word"""
    B = basic
    n, n_groups = 600, 6
    rng = random.Random(21)
    groups = [rng.randrange(n_groups) for _ in range(n)]
    weights = W.random_weights(22, n, 64)
    for k, w in enumerate(W.corner_weights(64) * 3):
        weights[(k * 23) % n] = w
    status = B["status"][:n]
    tallies, sums, counts, bad = run_device(torch, single5, B["d"][: n * single5.size], B["d_status"][:n], weights, 64, groups, n_groups)
    want, want_sums, want_counts, bad2 = W.expected(oracle, single5.op, B["ballots"][: n * single5.size], status, weights, groups, n_groups, 64)
    assert bad == (0, 0, 0) and bad2 == 0 and counts == want_counts
    assert sums == want_sums and all(s >> 64 for s in sums)
    assert bytes(tallies.cpu().numpy()) == want


# ------------------------------------------------------------------ 3. width sweep
@pytest.mark.parametrize("bits", W.WIDTHS)
def test_width_sweep_one_group_per_ballot(torch, eg, oracle, single5, basic, bits):
    """130 ballots, each its own group: some 1 200 lanes, ten per accepted ballot, corner weights at lanes 0 / 63 / 64 / last (the
    first, the seventh and the last accepted ballot); below 64 bits a few accepted ballots carry 2^W and 2^64 - 1 - counted in bad[2], absent from tallies, counts and sums, refused by the host form -
    and rejected ballots carry the same weights uncounted"""
    B = basic
    n = 130
    status = B["status"][:n]
    accepted = [b for b in range(n) if status[b] == 0]
    rejected = [b for b in range(n) if status[b] != 0]
    assert len(accepted) > 100 and len(rejected) >= 3
    lane_ballots = [accepted[0], accepted[6], accepted[-1]]     # groups of rejected ballots have no piece: piece = rank among the accepted
    weights = W.random_weights(300 + bits, n, bits)
    corners = W.corner_weights(bits)
    for k, b in enumerate(lane_ballots + accepted[10:15]):
        weights[b] = corners[(5 + k) % 8]                       # 2^W - 1 at lane 0, the alternating patterns at lanes 63 / 64 and the last
    over = []
    if bits < 64:
        over = accepted[20:24]
        for k, b in enumerate(over):
            weights[b] = (1 << bits, M64, (1 << bits) + 1, 1 << 63)[k]
        weights[rejected[0]], weights[rejected[1]] = 1 << bits, M64
    groups = list(range(n))
    tallies, sums, counts, bad = run_device(torch, single5, B["d"][: n * single5.size], B["d_status"][:n], weights, bits, groups, n)
    want, want_sums, want_counts, bad2 = W.expected(oracle, single5.op, B["ballots"][: n * single5.size], status, weights, groups, n, bits)
    assert bad == (0, 0, len(over)) and bad2 == len(over)
    assert counts == want_counts and sums == want_sums
    assert all(counts[b] == 0 and sums[b] == 0 for b in over + rejected)
    got = bytes(tallies.cpu().numpy())
    assert got == want
    assert all(got[b * 320:(b + 1) * 320] == bytes(320) for b in over + rejected)
    args = (B["ballots"][: n * single5.size], status, weights, groups, n)
    if over:
        with pytest.raises(eg.EgError, match=rf"error -3.*{len(over)} weight\(s\)"):
            single5.p.tally_weighted(*args, weight_bits=bits)
    else:
        assert single5.p.tally_weighted(*args, weight_bits=bits) == (want, want_sums, want_counts)


# ------------------------------------------------------------------ 4. seams
def test_group_sizes_at_the_seams_sorted_and_permuted(torch, oracle, single5):
    """groups of S1 - 1, S1, S1 + 1, S1 S2 - 1 and S1 S2 + 1 accepted ballots (and an empty one), weight_bits 3: sorted by group and
    randomly permuted give the same bytes, the oracle's"""
    sizes = {0: S1 - 1, 1: S1 + 1, 2: 0, 3: S1, 4: S1 * S2 - 1, 5: S1 * S2 + 1}
    groups = [g for g in sorted(sizes) for _ in range(sizes[g])]
    n = len(groups)
    d, ballots, status, d_status = verified(torch, single5, 1611, n)
    assert status == [0] * n
    weights = W.random_weights(4, n, 3)
    sorted_t, sums, counts, bad = run_device(torch, single5, d, d_status, weights, 3, groups, 6)
    assert bad == (0, 0, 0) and counts == [sizes[g] for g in range(6)]
    perm = list(range(n))
    random.Random(5).shuffle(perm)
    d_perm = d.view(n, single5.size)[torch.tensor(perm, device="cuda")].contiguous().view(-1)
    perm_t, perm_sums, perm_counts, bad = run_device(torch, single5, d_perm, d_status, [weights[i] for i in perm], 3, [groups[i] for i in perm], 6)
    assert bad == (0, 0, 0) and perm_counts == counts and perm_sums == sums
    assert torch.equal(sorted_t, perm_t)
    want, want_sums, _, _ = W.expected(oracle, single5.op, ballots, status, weights, groups, 6, 3)
    assert sums == want_sums and bytes(sorted_t.cpu().numpy()) == want


# ------------------------------------------------------------------ 5. the fourth level
def test_one_group_deep_enough_for_the_fourth_level(torch, eg, ctx, oracle, pk):
    """S1 S2^2 + 1 two-option ballots in one group need four levels of points and of weight sums; weight_bits 16; against the oracle"""
    shape = Shape(eg, ctx, oracle, pk, "single", 2)
    n = S1 * S2 * S2 + 1
    assert n < 100000 and G.depth(n, S1, S2) == 4
    d = shape.generate(torch, 1733, n)
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    shape.p.verify_batch_device(n, d.data_ptr(), status.data_ptr())
    shape.p.ctx.synchronize()
    assert int(status.abs().sum().item()) == 0
    weights = W.random_weights(16, n, 16)
    tallies, sums, counts, bad = run_device(torch, shape, d, status, weights, 16, None, 1)
    want, want_sums, _, _ = W.expected(oracle, shape.op, bytes(d.cpu().numpy()), [0] * n, weights, None, 1, 16)
    assert bad == (0, 0, 0) and counts == [n] and sums == want_sums == [sum(weights)]
    assert bytes(tallies.cpu().numpy()) == want
    shape.p.tally_reset()
    shape.p.close()


# ------------------------------------------------------------------ 6. edge ballots
def test_edge_ballots_with_top_weights(torch, eg, ctx, oracle):
    """the edge corpus (identity ciphertext components, cancelling pairs) under weights 2^63 and 2^64 - 1; the cancelling pair alone in
    group 2 under one weight: its random elements cancel to the identity in every slot"""
    fam = E.family("single5")
    p = fam.gpu_params(eg, ctx)
    try:
        pair = [e.ballot for e in fam.edges if e.name.startswith("cancel_")]
        rest = [e.ballot for e in fam.edges if not e.name.startswith("cancel_")]
        batch = rest + pair
        n = len(batch)
        ballots = b"".join(batch)
        status, _ = p.verify_batch(ballots, with_tally=False)
        assert status == [0] * n
        groups = [b % 2 for b in range(len(rest))] + [2, 2]
        weights = [(1 << 63, M64)[b % 3 == 0] for b in range(len(rest))] + [M64, M64]
        got, sums, counts = p.tally_weighted(ballots, status, weights, groups, 3, weight_bits=64)
        want, want_sums, want_counts, _ = W.expected(oracle, fam.oracle_params, ballots, status, weights, groups, 3, 64)
        assert (got, sums, counts) == (want, want_sums, want_counts) and counts[2] == 2 and sums[2] == 2 * M64
        cancelled = got[2 * 320:3 * 320]
        assert all(cancelled[64 * k:64 * k + 32] == E.IDENTITY for k in range(5))
        assert any(cancelled[64 * k + 32:64 * k + 64] == E.IDENTITY for k in range(5))
        assert any(any(ballots[b * fam.size + 32 * i:b * fam.size + 32 * i + 32] == E.IDENTITY for i in range(10)) for b in range(len(rest)))
    finally:
        p.close()


# ------------------------------------------------------------------ 7. other shapes
@pytest.mark.parametrize("kind,n_options,arg,n,n_groups", [("multi", 16, 3, 200, 4), ("qv", 5, 20, 300, 5)])
def test_other_election_shapes_against_the_oracle(torch, eg, ctx, oracle, pk, kind, n_options, arg, n, n_groups):
    """multi-choice 3-of-16 and quadratic voting 5 / 20 (partial ciphertexts between the tally items), 40-bit weights"""
    shape = Shape(eg, ctx, oracle, pk, kind, n_options, arg)
    d, ballots, status, d_status = verified(torch, shape, 1900 + n_options, n, range(5, n, 9))
    assert 0 < status.count(0) < n
    rng = random.Random(n)
    groups = [rng.randrange(n_groups) if rng.random() < 0.95 else NONE for _ in range(n)]
    weights = W.random_weights(n, n, 40)
    want, want_sums, want_counts, _ = W.expected(oracle, shape.op, ballots, status, weights, groups, n_groups, 40)
    assert shape.p.tally_weighted(ballots, status, weights, groups, n_groups, weight_bits=40) == (want, want_sums, want_counts)
    tallies, sums, counts, bad = run_device(torch, shape, d, d_status, weights, 40, groups, n_groups)
    assert bad == (0, 0, 0) and (bytes(tallies.cpu().numpy()), sums, counts) == (want, want_sums, want_counts)
    shape.p.close()


# ------------------------------------------------------------------ 8. linearity at size
def test_linearity_at_twenty_thousand_ballots(torch, eg, ctx, oracle, single5):
    """20 000 ballots in 100 groups: the tally under w1 + w2 is the slot-wise sum (eg_point_add_batch) of the tallies under w1 and w2;
    one group is also checked against the oracle"""
    n, n_groups = 20000, 100
    d = single5.generate(torch, 1808, n)
    tamper(torch, d, single5.size, range(7, n, 50), 3)
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    single5.p.verify_batch_device(n, d.data_ptr(), status.data_ptr())
    single5.p.ctx.synchronize()
    single5.p.tally_reset()
    rng = random.Random(8)
    groups = [rng.randrange(n_groups) for _ in range(n)]
    w1, w2 = W.random_weights(81, n, 32), W.random_weights(82, n, 20)
    t1, s1, c1, bad1 = run_device(torch, single5, d, status, w1, 32, groups, n_groups)
    t2, s2, c2, bad2 = run_device(torch, single5, d, status, w2, 20, groups, n_groups)
    t12, s12, c12, bad12 = run_device(torch, single5, d, status, [a + b for a, b in zip(w1, w2)], 33, groups, n_groups)
    assert bad1 == bad2 == bad12 == (0, 0, 0) and c1 == c2 == c12 and sum(c1) == int((status == 0).sum().item()) < n
    assert s12 == [a + b for a, b in zip(s1, s2)]
    added, ok = eg.Ristretto(ctx).element_add(bytes(t1.cpu().numpy()), bytes(t2.cpu().numpy()))
    assert set(ok) == {1} and added == bytes(t12.cpu().numpy())
    st = [s & 0xFFFFFFFF for s in status.cpu().tolist()]
    want, want_sums, _, _ = W.expected(oracle, single5.op, bytes(d.cpu().numpy()), st, w1, groups, n_groups, 32, only=[41])
    assert bytes(t1[41].cpu().numpy()) == want[41] and s1 == want_sums


# ------------------------------------------------------------------ 9. entry forms and statelessness
def test_entry_forms_statelessness_and_a_verify_call_alongside(torch, oracle, single5, basic, rejections):
    B = basic
    p, n, ng, size = single5.p, 500, B["n_groups"], single5.size
    status, groups = B["status"][:n], B["groups"][:n]
    d, d_status, ballots = B["d"][: n * size], B["d_status"][:n], B["ballots"][: n * size]
    weights = W.random_weights(9, n, 24)
    want, want_sums, want_counts, _ = W.expected(oracle, single5.op, ballots, status, weights, groups, ng, 24)
    p.tally_reset()
    verdicts = torch.zeros(n, dtype=torch.int32, device="cuda")
    p.verify_batch_device(n, d.data_ptr(), verdicts.data_ptr())
    p.ctx.synchronize()
    running = p.tally_encode()
    # a caller stream, twice, and without weight sums
    s = torch.cuda.Stream()
    first = run_device(torch, single5, d, d_status, weights, 24, groups, ng, stream=s.cuda_stream)
    second = run_device(torch, single5, d, d_status, weights, 24, groups, ng)
    third = run_device(torch, single5, d, d_status, weights, 24, groups, ng, with_sums=False)
    for t, sums, counts, bad in (first, second):
        assert bad == (0, 0, 0) and (bytes(t.cpu().numpy()), sums, counts) == (want, want_sums, want_counts)
    assert third[3] == (0, 0, 0) and bytes(third[0].cpu().numpy()) == want and third[1] == [(1 << 128) - 1] * ng      # sums left alone
    # host form against device form; groups == NULL against one group of everything
    assert p.tally_weighted(ballots, status, weights, groups, ng, weight_bits=24) == (want, want_sums, want_counts)
    whole, whole_sums, whole_counts, _ = W.expected(oracle, single5.op, ballots, status, weights, None, 1, 24)
    t, sums, counts, bad = run_device(torch, single5, d, d_status, weights, 24, None, 1)
    assert bad == (0, 0, 0) and (bytes(t.cpu().numpy()), sums, counts) == (whole, whole_sums, whole_counts)
    assert p.tally_weighted(ballots, status, weights, weight_bits=24) == (whole, whole_sums, whole_counts)
    assert p.tally_weighted(ballots, status, weights, [0] * n, 1, weight_bits=24) == (whole, whole_sums, whole_counts)
    # hostile group ids and a forged status word on accepted ballots
    accepted = [b for b in range(n) if status[b] == 0 and groups[b] != NONE]
    hostile_groups, hostile = list(groups), d.clone()
    hostile_groups[accepted[0]], hostile_groups[accepted[1]] = ng, 0xFFFFFFFE
    hostile.view(n, size)[accepted[2], 96:128] = torch.tensor(list(bytes.fromhex(rejections["non_element"]["hex"])), dtype=torch.uint8, device="cuda")
    _, _, counts, bad = run_device(torch, single5, hostile, d_status, weights, 24, hostile_groups, ng)
    assert bad == (2, 1, 0) and sum(counts) == len(accepted) - 2
    # beside a verify call on another thread
    errors, out = [], {}

    def verifier():
        try:
            vs = torch.cuda.Stream()
            st = torch.zeros(B["n"], dtype=torch.int32, device="cuda")
            p.verify_batch_device(B["n"], B["d"].data_ptr(), st.data_ptr(), stream=vs.cuda_stream)
            vs.synchronize()
            out["status"] = [x & 0xFFFFFFFF for x in st.cpu().tolist()]
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    def tallier():
        try:
            ts = torch.cuda.Stream()
            out["runs"] = [run_device(torch, single5, d, d_status, weights, 24, groups, ng, stream=ts.cuda_stream) for _ in range(3)]
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=verifier), threading.Thread(target=tallier)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert out["status"] == B["status"]
    for t, sums, counts, bad in out["runs"]:
        assert bad == (0, 0, 0) and (bytes(t.cpu().numpy()), sums, counts) == (want, want_sums, want_counts)
    # the running tally saw the verify calls only
    p.tally_reset()
    p.verify_batch_device(n, d.data_ptr(), verdicts.data_ptr())
    p.ctx.synchronize()
    before = p.tally_encode()
    assert before == running
    run_device(torch, single5, d, d_status, weights, 24, groups, ng)
    assert p.tally_weighted(ballots, status, weights, groups, ng, weight_bits=24)[0] == want
    assert p.tally_encode() == before
    p.tally_reset()


# ------------------------------------------------------------------ 10. refusals and scratch
def test_every_refusal_and_the_empty_calls(torch, eg, single5, basic):
    B = basic
    p, n = single5.p, 64
    d, st, gr, wt = B["d"], B["d_status"], u32(torch, [0] * n), u64(torch, [3] * n)
    scratch = torch.empty(p.tally_weighted_scratch_bytes(n, 4), dtype=torch.uint8, device="cuda")
    out = torch.zeros(4 * 320, dtype=torch.uint8, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    bad = torch.zeros(3, dtype=torch.int32, device="cuda")
    good = dict(n=n, d_ballots=d.data_ptr(), d_status=st.data_ptr(), d_weights=wt.data_ptr(), weight_bits=2, d_groups=gr.data_ptr(), n_groups=4,
                d_scratch=scratch.data_ptr(), d_tallies=out.data_ptr(), d_bad=bad.data_ptr(), d_weight_sums=sums.data_ptr())
    p.tally_weighted_device(**good)
    torch.cuda.synchronize()
    assert bad.cpu().tolist() == [0, 0, 0] and sums.cpu().tolist()[1] == 0 and sums.cpu().tolist()[0] == 3 * B["status"][:n].count(0)
    for change, message in ((dict(n_groups=0), "n_groups is 0"), (dict(n_groups=(1 << 24) + 1), "EG_TALLY_GROUPS_MAX"),
                            (dict(n=1 << 31), "2\\^31"), (dict(weight_bits=0), "weight_bits"), (dict(weight_bits=65), "weight_bits"),
                            (dict(weight_bits=-3), "weight_bits"), (dict(d_weights=0), "null weights"), (dict(d_groups=0), "n_groups must be 1"),
                            (dict(d_ballots=0), "null"), (dict(d_status=0), "null"), (dict(d_tallies=0), "null"), (dict(d_bad=0), "null"),
                            (dict(d_scratch=0), "null scratch"), (dict(d_ballots=d.data_ptr() + 4), "aligned"),
                            (dict(d_scratch=scratch.data_ptr() + 8), "aligned"), (dict(d_weights=wt.data_ptr() + 4), "8-byte aligned"),
                            (dict(d_weight_sums=sums.data_ptr() + 4), "8-byte aligned"), (dict(d_status=st.data_ptr() + 2), "misaligned")):
        with pytest.raises(eg.EgError, match=message):
            p.tally_weighted_device(**{**good, **change})
    assert p.tally_weighted_scratch_bytes(n, 0) == 0 == p.tally_weighted_scratch_bytes(1 << 31, 4) and p.tally_weighted_scratch_bytes(n, (1 << 24) + 1) == 0
    assert p.tally_weighted_scratch_bytes(n, 4) >= p.tally_grouped_scratch_bytes(n, 4) + 16 * (n // S1 + 4)
    ballots, status = B["ballots"][: n * single5.size], B["status"][:n]
    for kw, message in ((dict(n_groups=0), "n_groups is 0"), (dict(n_groups=(1 << 24) + 1), "EG_TALLY_GROUPS_MAX"), (dict(weight_bits=65), "weight_bits"),
                        (dict(groups=None, n_groups=2), "n_groups must be 1")):
        with pytest.raises(eg.EgError, match=message):
            p.tally_weighted(ballots, status, [3] * n, **{**dict(groups=[0] * n, n_groups=4, weight_bits=2), **kw})
    # n == 0, host and device, with and without groups
    assert p.tally_weighted(b"", [], [], [], 5) == (bytes(5 * 320), [0] * 5, [0] * 5)
    assert p.tally_weighted(b"", [], []) == (bytes(320), [0], [0])
    for groups, ng in (([], 3), (None, 1)):
        tallies, s, counts, b3 = run_device(torch, single5, None, None, [], 7, groups, ng)
        assert b3 == (0, 0, 0) and counts == [0] * ng == s and not bool(tallies.any().item())
    # no accepted ballot: nothing is looked at, whatever ids and weights say
    m = 500
    rejected = u32(torch, [1 + (b % 12) for b in range(m)])
    wild = [(b * 2654435761) & 0xFFFFFFFF for b in range(m)]
    tallies, s, counts, b3 = run_device(torch, single5, B["d"][: m * single5.size], rejected, [M64] * m, 5, wild, 4)
    assert b3 == (0, 0, 0) and counts == [0] * 4 == s and not bool(tallies.any().item())
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 11. the C++ example
def test_cpp_voting_example_weighted(tmp_path):
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "voting.cpp"),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    out = subprocess.run([str(exe), "--weighted", "200", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "199 of 200 ballots verified" in out.stdout
    # the example derives voter i's weight from its index and prints it beside the votes it cast: recompute the totals here
    rows = re.findall(r"^weighted voter #(\d+): weight (\d+), votes ([\d ]+), (accepted|rejected)$", out.stdout, re.M)
    assert len(rows) == 200 and sum(r[3] == "rejected" for r in rows) == 1 and len({r[1] for r in rows}) == 200
    want = [0] * 5
    for _, weight, votes, verdict in rows:
        votes = [int(v) for v in votes.split()]
        assert len(votes) == 5 and sum(votes) == 1
        if verdict == "accepted":
            want = [t + int(weight) * v for t, v in zip(want, votes)]
    got = [int(x) for x in re.findall(r"^weighted total of option #\d+: (\d+)$", out.stdout, re.M)]
    assert got == want and max(want) > 1 << 16
    assert int(re.search(r"^sum of the counted weights: (\d+)$", out.stdout, re.M).group(1)) == sum(want)
    assert "OK: the decrypted weighted totals equal the expected ones" in out.stdout
