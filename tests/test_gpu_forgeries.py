"""The reject path of every HIP verifier on WELL-FORMED forgeries (tests/forgery_cases.py): scalars and elements in their other
representations, algebraic neighbours of every item, sum-preserving pairs, true proofs of other statements, a lying prover,
transplants, two failures at once and challenges that differ from the recomputed one in a single word.  Each forgery sits next to
valid ballots.  The status words must equal the oracle's exactly (kind and detail), the tally of an election the oracle's tally over
the same verdicts, and the number of accepted ballots the number of valid ones placed.  Every number is the oracle's: no tolerances.
tests/test_forgeries_cpu.py shows that the oracle rejects every forgery, so an accepted one here is the engine's fault."""
import functools
import json
import random

import pytest

import forgery_cases as F

pytestmark = pytest.mark.gpu

PER_BATCH = 700                  # forgeries in one alternating batch: 2 x 700 + a wavefront + 1 ballots at the most


@pytest.fixture(scope="module")
def eg():
    import elastic_elgamal_amd as m

    return m


@pytest.fixture(scope="module")
def ctx(eg):
    c = eg.Context(0)
    yield c
    c.close()


def _ids(fams):
    return [f"{n}-{k}" for n, k in fams]


@functools.lru_cache(None)
def _want(name, key_name="golden"):
    """blob -> the oracle's status word, for the family's forgeries, its valid objects and its zero-randomness bases."""
    fam = F.family(name, key_name)
    want = {f.blob: s for f, s in zip(fam.forgeries, F.verdicts(name, key_name))}
    assert 0 not in want.values()
    want.update({v: 0 for v in fam.valid + fam.extra.get("word_bases", [])})
    return want


def _forged(fam):
    return [f.blob for f in fam.forgeries]


def _alternating(fam, phase):
    """Batches in which forgeries and valid objects alternate (phase 0: a forgery first, phase 1: a valid one first, and last), each
    followed by one whole wavefront of forgeries: over the two phases lanes 0, 63, 64 and the last lane see both kinds.  The
    zero-randomness bases of the one-word mutants ride along as valid objects."""
    forged = _forged(fam)
    valid = fam.valid + fam.extra.get("word_bases", [])
    out = []
    for lo in range(0, len(forged), PER_BATCH):
        part = forged[lo : lo + PER_BATCH]
        batch = []
        for i, f in enumerate(part):
            v = valid[(lo + i) % len(valid)]
            batch += [v, f] if phase else [f, v]
        batch += [forged[(lo + 5 * i) % len(forged)] for i in range(64)]
        if phase:
            batch.append(valid[0])
        out.append(batch)
    return out


def _check(fam, call, batch):
    """The status words (and the tally) `call` gives the batch == the oracle's; accepted == valid ones placed."""
    want_of = _want(fam.name, fam.key_name)
    want = [want_of[b] for b in batch]
    raw = b"".join(batch)
    got = call(raw)
    tally = None
    if fam.tallies:
        got, tally = got
    wrong = [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    names = {f.blob: f.name for f in fam.forgeries}
    assert not wrong, [(i, names.get(batch[i], "valid"), g, w) for i, g, w in wrong[:10]]
    assert len(got) == len(want)
    assert got.count(0) == sum(b not in names for b in batch) > 0
    if fam.tallies:
        assert tally == fam.tally(raw, want)


# ------------------------------------------------------------------ default batch entry, every family (standalone proofs included)
@pytest.mark.parametrize("name,key_name", F.FAMILIES, ids=_ids(F.FAMILIES))
def test_forgeries_beside_valid_ones_on_the_batch_entry(eg, ctx, name, key_name):
    fam = F.family(name, key_name)
    p = fam.gpu_params(eg, ctx)
    try:
        for phase in (0, 1):
            for batch in _alternating(fam, phase):
                assert len(batch) <= 2 * PER_BATCH + 65
                _check(fam, p.verify_batch, batch)
    finally:
        p.close()


@pytest.mark.parametrize("name", ["sumsq2", "commit_equiv"])
def test_true_proofs_under_a_label_one_byte_away(eg, ctx, name):
    """A verifier holding a label that differs in one byte rejects every valid proof of the family, and says what the oracle says."""
    fam = F.family(name)
    for label in F.OTHER_LABELS:
        other = fam.with_label(label)
        p = other.gpu_params(eg, ctx)
        try:
            want = [other.verify(v) for v in fam.valid]
            assert 0 not in want
            assert p.verify_batch(b"".join(fam.valid)) == want
        finally:
            p.close()


# ------------------------------------------------------------------ the fused tail's lane partners (single5)
def _halves(forged, valid, n_forged):
    pick = random.Random(386).sample(forged, n_forged) if n_forged < len(forged) else list(forged)
    return pick, [valid[i % len(valid)] for i in range(len(pick))]


@pytest.mark.parametrize("forged_first", [True, False])
def test_lane_partner_of_every_forgery_is_valid(eg, ctx, forged_first):
    """The fused tail gives a lane the ballots j and j + ceil(n / 2) of a chunk: every forgery with a valid partner, once as the
    first and once as the second ballot of its lane."""
    fam = F.family("single5")
    f, v = _halves(_forged(fam), fam.valid, len(fam.forgeries))
    p = fam.gpu_params(eg, ctx)
    try:
        _check(fam, p.verify_batch, f + v if forged_first else v + f)
    finally:
        p.close()


@pytest.mark.parametrize("forged_first", [True, False])
def test_lane_partners_on_both_sides_of_a_chunk_boundary(eg, ctx, monkeypatch, forged_first):
    """386 ballots with EG_CHUNK=256: a chunk of 256 (partners 128 apart) and one of 130 (65 apart), forgeries in both."""
    fam = F.family("single5")
    f, v = _halves(_forged(fam), fam.valid, 128 + 65)
    a, b = (f, v) if forged_first else (v, f)
    batch = a[:128] + b[:128] + a[128:] + b[128:]
    assert len(batch) == 386
    monkeypatch.setenv("EG_CHUNK", "256")                # read when the params object is made
    p = fam.gpu_params(eg, ctx)
    try:
        _check(fam, p.verify_batch, batch)
    finally:
        p.close()


# ------------------------------------------------------------------ the small entry: one workgroup a ballot
@pytest.mark.parametrize("name,key_name", [(n, "golden") for n in F.ELECTIONS] + [("single5", F.OTHER_KEY)],
                         ids=_ids([(n, "golden") for n in F.ELECTIONS] + [("single5", F.OTHER_KEY)]))
def test_forgeries_on_the_small_entry(eg, ctx, name, key_name):
    fam = F.family(name, key_name)
    p = fam.gpu_params(eg, ctx)
    try:
        for phase in (0, 1):
            for batch in _alternating(fam, phase):
                _check(fam, p.verify_small, batch)
    finally:
        p.close()


def test_one_forgery_alone_on_the_small_entry(eg, ctx):
    """verify_small with ONE ballot, for ten forgeries taken across the elections and the mutation families: no valid neighbour
    whose verdict could be the one reported."""
    picks = {"single5": ("rep_s+l@22", "pair_B0+G_B1-G", "word7@21"), "single9": ("rep_p-s@17", "lie_two_ones", "swap_ct_and_responses8_0"),
             "multi20": ("word0@40", "nbr_+2^224@40"), "qv4x12": ("two_credit_range_and_sumsq", "lie_vote3_above_range")}
    assert sum(len(v) for v in picks.values()) == 10
    for name, wanted in picks.items():
        fam = F.family(name)
        by_name = {f.name: f.blob for f in fam.forgeries}
        p = fam.gpu_params(eg, ctx)
        try:
            for nm in wanted:
                want = _want(name)[by_name[nm]]
                got, tally = p.verify_small(by_name[nm])
                assert got == [want] and want != 0, nm
                assert tally == fam.tally(by_name[nm], [want]), nm
            assert p.verify_small(fam.valid[0])[0] == [0]
        finally:
            p.close()


# ------------------------------------------------------------------ the other engines, single5 and qv4x12
OTHER = ["single5", "qv4x12"]


@pytest.mark.parametrize("group", ["1", "2"])
@pytest.mark.parametrize("name", ["single5", "multi20"])
def test_forgeries_on_the_ring_group_walk(eg, ctx, monkeypatch, name, group):
    """Only choice plans have a ring-group walk (host_plan.hpp: build_choice_plan), so multi20 stands in for quadratic voting."""
    monkeypatch.setenv("EG_RING_GROUP", group)           # read when the params object is made
    fam = F.family(name)
    assert eg.plan_describe(fam.kind, fam.n_options, fam.credits)["ring_group"] == int(group)
    p = fam.gpu_params(eg, ctx)
    try:
        for batch in _alternating(fam, 0):
            _check(fam, p.verify_batch, batch)
    finally:
        p.close()


def test_forgeries_on_wide_combs(eg, monkeypatch):
    """Wide fixed-base combs forced from the first ballot (EG_COMB_BIG_MIN=1, read when the context is made)."""
    monkeypatch.setenv("EG_COMB_BIG_MIN", "1")
    c = eg.Context(0)
    try:
        for name in OTHER:
            fam = F.family(name)
            p = fam.gpu_params(eg, c)
            try:
                for batch in _alternating(fam, 0):
                    _check(fam, p.verify_batch, batch)
            finally:
                p.close()
        assert c.comb_table_bits()[1] > 0
    finally:
        c.close()


@pytest.mark.parametrize("name", OTHER)
def test_forgeries_through_verify_json(eg, ctx, name):
    """The same ballots as JSON text in serde's layout (the native JSON entry packs them on host threads)."""
    from elastic_elgamal_amd import ingest, serde

    fam = F.family(name)
    if fam.kind == "qv":
        unpack = lambda b: ingest.unpack_qv_ballot(b, fam.n_options, fam.credits)           # noqa: E731
    else:
        unpack = lambda b: serde.unpack_encrypted_choice(b, fam.n_options, True)            # noqa: E731
    p = fam.gpu_params(eg, ctx)
    try:
        for batch in _alternating(fam, 1):
            _check(fam, lambda raw: p.verify_json(json.dumps([unpack(b) for b in batch])), batch)
    finally:
        p.close()
