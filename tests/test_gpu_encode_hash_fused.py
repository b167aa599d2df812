"""The fused stage tail (k_encode_hash: two ballots a lane, one batched inversion a pair, the stage's transcripts in the same
launch) against the CPU oracle: verdict words and the tally encoding of every case (tests/fused_tail_cases.py) must be the oracle's.
The plans the fused kernel does not serve (8 options, 3-of-16, quadratic voting) run the same checks through k_encode_batch + k_hash.

The library reads no switch that would put a single-choice plan back on the two kernels (its list of run-time knobs is pinned by
tests/test_abi_cpu.py), so there is no second run of the same call on them to compare with; the oracle is the reference.
For the same reason nothing here observes WHICH kernels ran: the checks hold for either tail, so they also pass on a library without
k_encode_hash.  That the single-choice plans do launch it is on record in profiles/r10_kernel_stats_*single.txt.

Lane j of the fused kernel owns ballots j and j + ceil(n / 2) of a chunk: in a batch of 65 ballot 0's partner is ballot 33.

The engine cuts a call into chunks that are whole multiples of its 256-ballot block, so 130 ballots are one chunk whatever
EG_CHUNK says (chunk_130 runs them with EG_CHUNK=65 all the same); the two-chunk cases therefore use 386 = 256 + 130 ballots with
EG_CHUNK=256: a full chunk and a 130-ballot one, one after the other on one work set (batch entry) and one on each work set (the
JSON entry, which always forks)."""
import json

import pytest

import fused_tail_cases as F

pytestmark = pytest.mark.gpu


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
def wanted():
    """name -> (status words, tally hex) by the oracle."""
    out = {}
    for name, (_, ballots, _, _) in F.cases().items():
        fam = F.family_of(name)
        raw = b"".join(ballots)
        st = list(fam.oracle_params.verify_batch(raw))
        out[name] = (st, fam.tally(raw, st).hex())
    return out


def _run(eg, ctx, wanted, name):
    got = F.run_case(eg, ctx, name)
    assert got[0] == wanted[name][0], name
    assert got[1] == wanted[name][1], name
    return got[0]


@pytest.mark.parametrize("n", F.SIZES)
def test_batch_sizes(eg, ctx, wanted, n):
    """One lane and one ballot; a pair; an unpaired last lane (odd n); pairs whose halves sit in different wavefronts (129) and
    blocks with a partial last block (257)."""
    st = _run(eg, ctx, wanted, f"size{n}")
    assert st == [0] * n


@pytest.mark.parametrize("name,fused", [("single2", True), ("single7", True), ("single8", False), ("multi3of16", False), ("qv5x20", False)])
def test_option_counts(eg, ctx, wanted, name, fused):
    """2 and 7 options run the fused kernel with 2 x 4 and 2 x 16 commitments in the batch (the limit); 8 options, 3-of-16 and
    quadratic voting keep the two kernels.  65 ballots, one of them tampered."""
    fam = F.family_of(f"options_{name}")
    d = eg.plan_describe(fam.kind, fam.n_options, fam.credits)
    per_stage = json.loads(d["jobs_per_stage"]) if isinstance(d["jobs_per_stage"], str) else d["jobs_per_stage"]
    assert (fam.kind == "single" and max(per_stage) - d["plain_encodes"] <= 16) == fused
    st = _run(eg, ctx, wanted, f"options_{name}")
    assert [i for i, s in enumerate(st) if s] == [5]


@pytest.mark.parametrize("tag,bad", [("first", [0]), ("partner", [33]), ("both", [0, 33])])
def test_tampered_partner(eg, ctx, wanted, tag, bad):
    """One response bit flipped in ballot 0, in its partner 33, in both: the other ballot of the lane is accepted and the tampered
    one gets the oracle's error word."""
    st = _run(eg, ctx, wanted, f"tampered_{tag}")
    assert [i for i, s in enumerate(st) if s] == bad


@pytest.mark.parametrize("name", ["edge_first", "edge_second", "edge_both", "edge_odd"])
def test_guard_ballots_leave_their_partners_alone(eg, ctx, wanted, name):
    """Valid ballots with identity commitments (the encoder swaps their vanishing denominator for 1 and flags the commitment) paired
    with ordinary ballots, either way round, with each other, and alone in the last lane: all accepted."""
    assert len(F.guard_edges(F.family_of(name))) >= 4
    st = _run(eg, ctx, wanted, name)
    assert st == [0] * len(st)


@pytest.mark.parametrize("name", ["chunk_130", "chunk_386", "chunk_386_two_sets"])
def test_chunks(eg, ctx, wanted, name):
    """Chunks of 256 + 130 ballots (see the module docstring) with the tally on, on one work set and on two."""
    st = _run(eg, ctx, wanted, name)
    assert len(st) == len(F.cases()[name][1])
