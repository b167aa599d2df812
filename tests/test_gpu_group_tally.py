"""The per-group tally (eg_*_tally_grouped[_device]) on the GPU: ballots from the GPU generators, verdicts from the batch entry, every
group's tally against the oracle's tally of its subset (or against the ballots' own ciphertext bytes, or against the batch entry's
tally_out where the group is too large for the oracle to be quick), the seams of the piece sizes, the fourth level, hostile group ids
and forged status words, entry forms, concurrency with verify calls and an open JSON stream, slabs merged with eg_points_sum_device,
and the C++ example."""
import random
import statistics
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import group_tally_cases as G

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NONE = G.GROUP_NONE
S1, S2 = G.piece_sizes()


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


def run_device(torch, shape, d_ballots, d_status, groups, n_groups, stream=0, d_groups=None):
    """the device entry with buffers of its own -> (tallies tensor [n_groups, 64 n_options], counts list, bad tuple)"""
    p, n = shape.p, len(groups)
    d_groups = u32(torch, groups) if d_groups is None else d_groups
    scratch = torch.empty(max(p.tally_grouped_scratch_bytes(n, n_groups), 16), dtype=torch.uint8, device="cuda")
    tallies = torch.full((n_groups, 64 * shape.n_options), 0xAB, dtype=torch.uint8, device="cuda")
    counts = torch.full((n_groups,), -1, dtype=torch.int32, device="cuda")
    bad = torch.full((2,), 77, dtype=torch.int32, device="cuda")          # the library WRITES both words
    torch.cuda.synchronize()
    p.tally_grouped_device(n, d_ballots.data_ptr() if n else 0, d_status.data_ptr() if n else 0, d_groups.data_ptr() if n else 0, n_groups,
                           scratch.data_ptr(), tallies.data_ptr(), bad.data_ptr(), d_counts=counts.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return tallies, counts.cpu().tolist(), tuple(bad.cpu().tolist())


def tamper(torch, d_ballots, size, which, seed):
    """flips one bit of a scalar or point of every ballot in `which`"""
    rng = random.Random(seed)
    view = d_ballots.view(-1, size)
    for b in which:
        view[b, 32 * rng.randrange(size // 32) + rng.randrange(32)] ^= 1 << rng.randrange(8)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def basic(torch, single5):
    """3 000 five-option ballots, a tenth tampered, verified by the batch entry; 7 groups of which group 3 is empty, 50 ballots in none"""
    n, n_groups = 3000, 7
    d = single5.generate(torch, 501, n)
    tamper(torch, d, single5.size, range(3, n, 10), 9)
    ballots = bytes(d.cpu().numpy())
    status, tally_out = single5.p.verify_batch(ballots)
    assert 2500 < status.count(0) <= 2700
    rng = random.Random(77)
    groups = [rng.choice((0, 1, 2, 4, 5, 6)) for _ in range(n)]
    for b in rng.sample(range(n), 50):
        groups[b] = NONE
    want, want_counts = G.expected(single5.op, ballots, status, groups, n_groups)
    return dict(n=n, n_groups=n_groups, d=d, ballots=ballots, status=status, d_status=u32(torch, status), tally_out=tally_out,
                groups=groups, want=want, want_counts=want_counts)


# ------------------------------------------------------------------ basic
def test_every_group_equals_the_oracle_tally_of_its_subset(torch, ctx, single5, basic):
    B = basic
    tallies, counts = single5.p.tally_grouped(B["ballots"], B["status"], B["groups"], B["n_groups"])
    assert counts == B["want_counts"] and counts[3] == 0 and sum(counts) == sum(1 for s, g in zip(B["status"], B["groups"]) if s == 0 and g != NONE)
    assert tallies == B["want"]
    assert tallies[3 * 320:4 * 320] == bytes(320)
    # the groups and the ballots in no group add up to the verify call's own tally (eg_points_sum_device)
    rest = [0 if g == NONE else NONE for g in B["groups"]]
    none_tally, none_count = single5.p.tally_grouped(B["ballots"], B["status"], rest, 1)
    assert 0 < none_count[0] <= 50
    parts = torch.frombuffer(bytearray(tallies + none_tally), dtype=torch.uint8).cuda()
    out = torch.zeros(320, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.points_sum_device(B["n_groups"] + 1, 10, parts.data_ptr(), out.data_ptr(), d_bad=bad.data_ptr())
    torch.cuda.synchronize()
    assert int(bad.item()) == 0 and bytes(out.cpu().numpy()) == B["tally_out"]


# ------------------------------------------------------------------ seams of the piece sizes
def test_group_sizes_at_the_seams_sorted_and_permuted(torch, single5):
    """one call with groups of 0, 1, S1 - 1, S1, S1 + 1, S1 S2 - 1, S1 S2 and S1 S2 + 1 accepted ballots; sorted by group (boundaries at
    ballots 63 / 64 and at the last ballot) and randomly permuted give the same bytes, which are the oracle's"""
    sizes = {0: S1 - 1, 1: S1 + 1, 2: 0, 3: 1, 4: S1, 5: S1 * S2 - 1, 6: S1 * S2, 7: S1 * S2 + 1}
    assert sizes[0] + sizes[1] == 64
    groups = [g for g in sorted(sizes) for _ in range(sizes[g])]
    n = len(groups)
    assert groups[63] != groups[64] and groups[-1] == 7
    d = single5.generate(torch, 611, n)
    ballots = bytes(d.cpu().numpy())
    status, _ = single5.p.verify_batch(ballots, with_tally=False)
    assert status == [0] * n
    d_status = u32(torch, status)
    sorted_t, counts, bad = run_device(torch, single5, d, d_status, groups, 8)
    assert bad == (0, 0) and counts == [sizes[g] for g in range(8)]
    perm = list(range(n))
    random.Random(5).shuffle(perm)
    d_perm = d.view(n, single5.size)[torch.tensor(perm, device="cuda")].contiguous().view(-1)
    perm_t, perm_counts, bad = run_device(torch, single5, d_perm, d_status, [groups[i] for i in perm], 8)
    assert bad == (0, 0) and perm_counts == counts
    assert torch.equal(sorted_t, perm_t)
    want, _ = G.expected(single5.op, ballots, status, groups, 8)
    assert bytes(sorted_t.cpu().numpy()) == want


# ------------------------------------------------------------------ depth
def test_one_group_deep_enough_for_the_fourth_level(torch, single5):
    """S1 S2^2 + 1 accepted ballots in one group need four levels; that group's tally is the batch entry's own tally of exactly those
    ballots, the small groups beside it are the oracle's"""
    big = S1 * S2 * S2 + 1
    assert big < 100000 and G.depth(big, S1, S2) == 4
    small = [3, 1, S1 + 2]
    n = big + sum(small)
    d = single5.generate(torch, 733, n)
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    single5.p.tally_reset()
    single5.p.verify_batch_device(big, d.data_ptr(), status.data_ptr())
    single5.p.ctx.synchronize()
    want_big = single5.p.tally_encode()
    single5.p.verify_batch_device(n - big, d.data_ptr() + big * single5.size, status.data_ptr() + 4 * big)
    single5.p.ctx.synchronize()
    assert int(status.abs().sum().item()) == 0
    groups = [2] * big + [0] * small[0] + [1] * small[1] + [3] * small[2]
    order = list(range(n))
    random.Random(8).shuffle(order)
    d_mixed = d.view(n, single5.size)[torch.tensor(order, device="cuda")].contiguous().view(-1)
    tallies, counts, bad = run_device(torch, single5, d_mixed, status, [groups[i] for i in order], 4)
    assert bad == (0, 0) and counts == [small[0], small[1], big, small[2]]
    got = bytes(tallies.cpu().numpy())
    assert got[2 * 320:3 * 320] == want_big
    tail = bytes(d[big * single5.size:].cpu().numpy())
    want_small, _ = G.expected(single5.op, tail, [0] * (n - big), [g if g < 2 else g - 1 for g in groups[big:]], 3)
    assert got[:640] == want_small[:640] and got[960:] == want_small[640:]


# ------------------------------------------------------------------ extremes
def test_one_group_and_one_group_per_ballot(torch, single5, basic):
    B = basic
    tallies, counts, bad = run_device(torch, single5, B["d"], B["d_status"], [0] * B["n"], 1)
    assert bad == (0, 0) and counts == [B["status"].count(0)]
    assert bytes(tallies.cpu().numpy()) == B["tally_out"]
    # every ballot its own group: an accepted ballot's tally is its own ciphertexts, byte for byte
    n = 1000
    tallies, counts, bad = run_device(torch, single5, B["d"][: n * single5.size], B["d_status"][:n], list(range(n)), n)
    assert bad == (0, 0) and counts == [int(s == 0) for s in B["status"][:n]]
    got = bytes(tallies.cpu().numpy())
    for b in range(n):
        want = B["ballots"][b * single5.size:b * single5.size + 320] if B["status"][b] == 0 else bytes(320)
        assert got[b * 320:(b + 1) * 320] == want, b


def test_a_million_groups_and_three_hundred_ballots(torch, single5, basic):
    B = basic
    n, n_groups = 300, 1 << 20
    rng = random.Random(20)
    groups = rng.sample(range(n_groups), n - 20) + [n_groups - 1, 0] * 10            # the two ends hold ten ballots each
    tallies, counts, bad = run_device(torch, single5, B["d"][: n * single5.size], B["d_status"][:n], groups, n_groups)
    assert bad == (0, 0)
    occupied = sorted({g for g, s in zip(groups, B["status"][:n]) if s == 0})
    want, want_counts = G.expected(single5.op, B["ballots"][: n * single5.size], B["status"][:n], groups, n_groups, only=occupied)
    rows = tallies[torch.tensor(occupied, device="cuda")].cpu().numpy()
    for i, g in enumerate(occupied):
        assert bytes(rows[i]) == want[g] and counts[g] == want_counts[g], g
    assert sum(counts) == B["status"][:n].count(0) and counts[0] + counts[n_groups - 1] > 10
    empties = [g for g in rng.sample(range(n_groups), 1100) if g not in set(groups)][:1000]
    assert not bool(tallies[torch.tensor(empties, device="cuda")].any().item())
    assert int(tallies.any(dim=1).sum().item()) == len(occupied)                       # and nothing else anywhere


def test_no_ballots_and_no_accepted_ballots(torch, single5, basic):
    B = basic
    tallies, counts = single5.p.tally_grouped(b"", [], [], 5)
    assert tallies == bytes(5 * 320) and counts == [0] * 5
    tallies, counts, bad = run_device(torch, single5, None, None, [], 3)
    assert bad == (0, 0) and counts == [0] * 3 and not bool(tallies.any().item())
    # every ballot rejected: nothing is looked at, whatever the group ids say
    n = 500
    rejected = u32(torch, [1 + (b % 12) for b in range(n)])
    wild = [(b * 2654435761) & 0xFFFFFFFF for b in range(n)]
    tallies, counts, bad = run_device(torch, single5, B["d"][: n * single5.size], rejected, wild, 4)
    assert bad == (0, 0) and counts == [0] * 4 and not bool(tallies.any().item())


# ------------------------------------------------------------------ other shapes
@pytest.mark.parametrize("kind,n_options,arg,n,n_groups", [("multi", 16, 3, 500, 5), ("qv", 5, 20, 500, 5), ("qv", 3, 10000, 100, 3)])
def test_other_election_shapes_against_the_oracle(torch, eg, ctx, oracle, pk, kind, n_options, arg, n, n_groups):
    """multi-choice 3-of-16 and quadratic voting: the tally items are not the first items of the ballot (QV (3, 10^4) has several
    partial ciphertexts between two of them)"""
    shape = Shape(eg, ctx, oracle, pk, kind, n_options, arg)
    d = shape.generate(torch, 900 + n_options, n)
    tamper(torch, d, shape.size, range(5, n, 9), 4)
    ballots = bytes(d.cpu().numpy())
    status, tally_out = shape.p.verify_batch(ballots)
    assert 0 < status.count(0) < n
    rng = random.Random(n)
    groups = [rng.randrange(n_groups) if rng.random() < 0.95 else NONE for _ in range(n)]
    want, want_counts = G.expected(shape.op, ballots, status, groups, n_groups)
    tallies, counts = shape.p.tally_grouped(ballots, status, groups, n_groups)
    assert counts == want_counts and tallies == want
    dev, dev_counts, bad = run_device(torch, shape, d, u32(torch, status), groups, n_groups)
    assert bad == (0, 0) and dev_counts == counts and bytes(dev.cpu().numpy()) == tallies
    whole, _ = shape.p.tally_grouped(ballots, status, [0] * n, 1)
    assert whole == tally_out == shape.op.tally(ballots, status)
    shape.p.close()


# ------------------------------------------------------------------ hostile inputs
def test_hostile_group_ids_and_forged_status_words(torch, eg, single5, basic, rejections):
    B = basic
    n, n_groups, size = 600, 7, single5.size
    status, groups = list(B["status"][:n]), [g if g == NONE else g % n_groups for g in B["groups"][:n]]
    accepted = [b for b in range(n) if status[b] == 0 and groups[b] != NONE]
    rejected = [b for b in range(n) if status[b] != 0]
    non_element = list(bytes.fromhex(rejections["non_element"]["hex"]))
    bad_scalar = list(bytes.fromhex(rejections["non_canonical_scalar"]["hex"]))
    d = B["d"][: n * size].clone()
    view = d.view(n, size)
    # on rejected ballots: never looked at
    groups[rejected[0]], groups[rejected[1]] = n_groups, 0xFFFFFFFE
    view[rejected[2], 96:128] = torch.tensor(non_element, dtype=torch.uint8, device="cuda")
    ballots = bytes(d.cpu().numpy())
    want, want_counts = G.expected(single5.op, ballots, status, groups, n_groups)
    tallies, counts, bad = run_device(torch, single5, d, u32(torch, status), groups, n_groups)
    assert bad == (0, 0) and counts == want_counts and bytes(tallies.cpu().numpy()) == want
    assert single5.p.tally_grouped(ballots, status, groups, n_groups) == (want, want_counts)
    # on accepted ballots: two ids out of range, one undecodable tally point, one non-canonical scalar at a non-tally item
    a, b, c, e = accepted[:4]
    groups[a], groups[b] = n_groups, 0xFFFFFFFE
    view[c, 96:128] = torch.tensor(non_element, dtype=torch.uint8, device="cuda")                 # tally item 3
    view[e, 32 * 12:32 * 13] = torch.tensor(bad_scalar, dtype=torch.uint8, device="cuda")         # a ring response: not a tally item
    ballots = bytes(d.cpu().numpy())
    assert [single5.op.verify(ballots[x * size:(x + 1) * size]) != 0 for x in (c, e)] == [True, True]   # forged: no verifier accepts them
    tallies, counts, bad = run_device(torch, single5, d, u32(torch, status), groups, n_groups)
    assert bad == (2, 1)
    assert counts == [sum(1 for x in range(n) if status[x] == 0 and groups[x] == g) for g in range(n_groups)]   # the two strays are in no group
    others = [g for g in range(n_groups) if g != groups[c]]               # (the group of the undecodable point is to be discarded)
    want, _ = G.expected(single5.op, ballots, status, groups, n_groups, only=others)
    got = bytes(tallies.cpu().numpy())
    for g in others:
        assert got[g * 320:(g + 1) * 320] == want[g], g
    with pytest.raises(eg.EgError, match="error -3.*2 accepted ballot.*1 tally point"):
        single5.p.tally_grouped(ballots, status, groups, n_groups)
    # the device is healthy: a normal call right after is exact
    tallies, counts = single5.p.tally_grouped(B["ballots"], B["status"], B["groups"], B["n_groups"])
    assert tallies == B["want"] and counts == B["want_counts"]


def test_every_refusal(torch, eg, single5, basic):
    B = basic
    p, n = single5.p, 64
    d, st, gr = B["d"], B["d_status"], u32(torch, [0] * n)
    scratch = torch.empty(p.tally_grouped_scratch_bytes(n, 4), dtype=torch.uint8, device="cuda")
    out = torch.zeros(4 * 320, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(2, dtype=torch.int32, device="cuda")
    good = dict(n=n, d_ballots=d.data_ptr(), d_status=st.data_ptr(), d_groups=gr.data_ptr(), n_groups=4, d_scratch=scratch.data_ptr(),
                d_tallies=out.data_ptr(), d_bad=bad.data_ptr())
    p.tally_grouped_device(**good)
    torch.cuda.synchronize()
    for change, message in ((dict(n_groups=0), "n_groups is 0"), (dict(n_groups=(1 << 24) + 1), "EG_TALLY_GROUPS_MAX"),
                            (dict(n=1 << 31), "2\\^31"), (dict(d_ballots=0), "null"), (dict(d_status=0), "null"), (dict(d_groups=0), "null"),
                            (dict(d_tallies=0), "null"), (dict(d_bad=0), "null"), (dict(d_scratch=0), "null scratch"),
                            (dict(d_ballots=d.data_ptr() + 4), "aligned"), (dict(d_scratch=scratch.data_ptr() + 8), "aligned"),
                            (dict(d_status=st.data_ptr() + 2), "misaligned")):
        with pytest.raises(eg.EgError, match=message):
            p.tally_grouped_device(**{**good, **change})
    assert p.tally_grouped_scratch_bytes(n, 0) == 0 == p.tally_grouped_scratch_bytes(1 << 31, 4) and p.tally_grouped_scratch_bytes(n, (1 << 24) + 1) == 0
    for ng, message in ((0, "n_groups is 0"), ((1 << 24) + 1, "EG_TALLY_GROUPS_MAX")):
        with pytest.raises(eg.EgError, match=message):
            p.tally_grouped(B["ballots"][: n * single5.size], B["status"][:n], [0] * n, ng)
    torch.cuda.synchronize()
    assert p.tally_grouped(B["ballots"], B["status"], B["groups"], B["n_groups"])[0] == B["want"]


# ------------------------------------------------------------------ entries and concurrency
def test_entry_forms_agree_on_a_caller_stream_and_twice(torch, single5, basic):
    B = basic
    s = torch.cuda.Stream()
    first, counts, bad = run_device(torch, single5, B["d"], B["d_status"], B["groups"], B["n_groups"], stream=s.cuda_stream)
    second, counts2, _ = run_device(torch, single5, B["d"], B["d_status"], B["groups"], B["n_groups"])
    assert bad == (0, 0) and counts == counts2 == B["want_counts"]
    assert torch.equal(first, second) and bytes(first.cpu().numpy()) == B["want"]
    assert single5.p.tally_grouped(B["ballots"], B["status"], B["groups"], B["n_groups"]) == (B["want"], B["want_counts"])


def test_grouped_passes_beside_verify_calls_and_an_open_json_stream(torch, ctx, single5, basic):
    """two threads run the grouped pass while a third verifies on the same params object: every result exact, and the running tally the
    exact sum of the verify calls; with a JSON stream of the params object open the pass still answers"""
    B = basic
    p, rounds, errors, results = single5.p, 3, [], {}
    p.tally_reset()

    def grouper(k):
        try:
            s = torch.cuda.Stream()
            groups = B["groups"] if k == 0 else [g if g == NONE else (g + k) % B["n_groups"] for g in B["groups"]]
            results[k] = (groups, [run_device(torch, single5, B["d"], B["d_status"], groups, B["n_groups"], stream=s.cuda_stream) for _ in range(rounds)])
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    def verifier():
        try:
            s = torch.cuda.Stream()
            st = torch.zeros(B["n"], dtype=torch.int32, device="cuda")
            for _ in range(rounds):
                p.verify_batch_device(B["n"], B["d"].data_ptr(), st.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            results["status"] = st.cpu().tolist()
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=grouper, args=(0,)), threading.Thread(target=grouper, args=(1,)), threading.Thread(target=verifier)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert results["status"] == [s if s < 1 << 31 else s - (1 << 32) for s in B["status"]]
    for k in (0, 1):
        groups, runs = results[k]
        want, want_counts = (B["want"], B["want_counts"]) if k == 0 else G.expected(single5.op, B["ballots"], B["status"], groups, B["n_groups"])
        for tallies, counts, bad in runs:
            assert bad == (0, 0) and counts == want_counts and bytes(tallies.cpu().numpy()) == want
    parts = torch.frombuffer(bytearray(B["tally_out"] * rounds), dtype=torch.uint8).cuda()
    out = torch.zeros(320, dtype=torch.uint8, device="cuda")
    ctx.points_sum_device(rounds, 10, parts.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert p.tally_encode() == bytes(out.cpu().numpy())
    p.tally_reset()
    stream = p.json_stream()
    try:
        assert p.tally_grouped(B["ballots"], B["status"], B["groups"], B["n_groups"]) == (B["want"], B["want_counts"])
        tallies, counts, bad = run_device(torch, single5, B["d"], B["d_status"], B["groups"], B["n_groups"])
        assert bad == (0, 0) and bytes(tallies.cpu().numpy()) == B["want"]
    finally:
        stream.abort()


# ------------------------------------------------------------------ slabs
def test_two_unequal_slabs_merge_to_the_whole(torch, ctx, single5, basic):
    B = basic
    cut, n, ng, size = 1100, B["n"], B["n_groups"], single5.size
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        t, _, bad = run_device(torch, single5, B["d"][lo * size:hi * size], B["d_status"][lo:hi], B["groups"][lo:hi], ng)
        assert bad == (0, 0)
        parts.append(t.view(-1))
    both = torch.cat(parts)
    out = torch.zeros(ng * 320, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.points_sum_device(2, ng * 10, both.data_ptr(), out.data_ptr(), d_bad=bad.data_ptr())
    torch.cuda.synchronize()
    assert int(bad.item()) == 0 and bytes(out.cpu().numpy()) == B["want"]


# ------------------------------------------------------------------ the C++ example
def test_cpp_voting_example_by_precinct(tmp_path):
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "voting.cpp"),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    out = subprocess.run([str(exe), "--precincts", "3", "200", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "199 of 200 ballots verified" in out.stdout
    assert all(f"precinct #{k}: " in out.stdout for k in (1, 2, 3)) and "precinct #4" not in out.stdout
    accepted = [int(x) for x in __import__("re").findall(r"precinct #\d+: (\d+) accepted ballots", out.stdout)]
    assert accepted == [66, 67, 66]                                  # voter #4 (index 3, precinct 1) is the forged one
    assert "precinct totals add up to the overall totals" in out.stdout
    assert "OK: the decrypted totals equal the expected ones" in out.stdout
    out = subprocess.run([str(exe), "--qv", "--precincts", "4", "60", "3", "20", "11"], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "precinct totals add up to the overall totals" in out.stdout


# ------------------------------------------------------------------ a loose guard against an accidental O(n groups) design
def test_grouped_pass_is_cheaper_than_verifying(torch, single5):
    """n = 2^18 ballots in 4 096 groups: the grouped pass takes no longer than the batch verify call of the same ballots in the same
    process (warm, median of three, HIP events).  The pass decodes 2 n_options points per accepted ballot; verifying a ballot costs
    some twenty times that."""
    n, n_groups = 1 << 18, 4096
    p = single5.p
    d = single5.generate(torch, 4242, n)
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(3)
    d_groups = u32(torch, rng.integers(0, n_groups, n))
    scratch = torch.empty(p.tally_grouped_scratch_bytes(n, n_groups), dtype=torch.uint8, device="cuda")
    tallies = torch.zeros(n_groups * 320, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(2, dtype=torch.int32, device="cuda")
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
    grouped_ms = timed(lambda: p.tally_grouped_device(n, d.data_ptr(), status.data_ptr(), d_groups.data_ptr(), n_groups, scratch.data_ptr(),
                                                      tallies.data_ptr(), bad.data_ptr(), stream=stream))
    print(f"n = 2^18, 4096 groups: grouped pass {grouped_ms:.3f} ms, batch verify {verify_ms:.3f} ms")
    assert bad.cpu().tolist() == [0, 0] and int(status.abs().sum().item()) == 0
    assert grouped_ms <= verify_ms
    p.tally_reset()
