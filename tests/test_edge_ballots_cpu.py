"""The edge corpus (tests/edge_ballots.py) and the oracle's scripted randomness, without a GPU: the oracle accepts every corpus
ballot, its verifier counters show that each one reaches the edge it is named after, a one-bit tamper of each is rejected, and a
script that pins nothing leaves the provers' output byte-identical."""
import pytest

import edge_ballots as E


@pytest.mark.parametrize("key_name", E.KEY_NAMES)
@pytest.mark.parametrize("fam_name", E.FAMILY_NAMES)
def test_corpus_is_accepted_and_reaches_its_edges(oracle, fam_name, key_name):
    fam = E.family(fam_name, key_name)
    assert len(fam.edges) >= 5
    assert len({e.ballot for e in fam.edges}) == len(fam.edges)
    for e in fam.edges:
        assert all(len(x.ballot) == fam.size for x in fam.edges)
        oracle.diag_reset()
        assert fam.verify(e.ballot) == 0, e.name
        got = oracle.diag()
        for what, at_least in e.needs.items():
            assert got[what] >= at_least, (e.name, what, got)
        for item, value in e.items.items():
            assert e.ballot[32 * item : 32 * item + 32] == value, (e.name, item)
    # every family reaches identity elements somewhere, and the corner-response ballots carry the corners they were built for
    assert any(e.needs for e in fam.edges)


def test_corners_cover_both_comb_widths_and_the_halved_form():
    cs = set(E.corner_scalars())
    L = E.L
    assert {0, 1, L - 1, 2, L - 2} <= cs
    for bits, windows in ((20, 13), (24, 11)):
        for w in range(windows):
            for d in (1, 2**bits - 1, 2 ** (bits - 1)):
                c = (d << (bits * w)) % L
                assert c in cs and 2 * c % L in cs
    # the golden key's 2- and 5-option elections carry every corner as a response
    for name in ("single2", "single5"):
        fam = E.family(name)
        carried = {int.from_bytes(v, "little") for e in fam.edges for v in e.items.values()}
        assert cs <= carried, name


def test_counters_stay_zero_on_ordinary_ballots(oracle, golden):
    import base64

    pk = base64.urlsafe_b64decode(golden["public_key_b64"] + "=" * (-len(golden["public_key_b64"]) % 4))
    op = oracle.ChoiceParams(pk, 5, True)
    ballots = op.generate_batch(5, 0, 20, threads=1)
    oracle.diag_reset()
    assert [op.verify(ballots[i * op.ballot_size : (i + 1) * op.ballot_size]) for i in range(20)] == [0] * 20
    assert oracle.diag() == {"commitment": 0, "ciphertext": 0, "base": 0}


@pytest.mark.parametrize("fam_name", E.FAMILY_NAMES)
def test_tampered_twins_are_rejected(oracle, fam_name):
    """A flipped bit in the challenge is rejected for every corpus ballot; a flipped bit anywhere is rejected for most of them (an
    r = 0 ring leaves some free responses unbound, edge_ballots.py)."""
    for key_name in ("golden", "-G"):
        fam = E.family(fam_name, key_name)
        anywhere = []
        for i, e in enumerate(fam.edges):
            bad = E.tamper(e.ballot, i, fam.challenge_item)
            assert bad != e.ballot
            assert fam.verify(bad) != 0, (key_name, e.name)
            anywhere.append(fam.verify(E.tamper(e.ballot, i)))
        assert anywhere.count(0) <= len(anywhere) // 2, anywhere


@pytest.mark.parametrize("fam_name", ["single5", "multi3of16", "qv5x20"])
def test_cancelling_pairs_tally_to_the_identity(oracle, fam_name):
    fam = E.family(fam_name)
    pair = [e for e in fam.edges if e.name.startswith("cancel_")]
    assert len(pair) == 2
    t = fam.tally(pair[0].ballot + pair[1].ballot, [0, 0])
    for k in range(fam.n_options):
        assert t[64 * k : 64 * k + 32] == E.IDENTITY                # R of every slot cancels
    zero_slots = [k for k in range(fam.n_options) if t[64 * k + 32 : 64 * k + 64] == E.IDENTITY]
    assert zero_slots, "no slot cancels completely"


def test_unpinned_script_leaves_the_stream_unchanged(oracle, golden):
    o = oracle
    _, pk, _ = o.keypair_from_seed(12345)
    op, oq, k = o.ChoiceParams(pk, 5, True), o.QvParams(pk, 5, 20), o.PublicKey(pk)
    pr = o.PreparedRange(100)
    makers = {
        "choice": lambda r: op.new_ballot([0, 0, 1, 0, 0], r),
        "multi": lambda r: o.ChoiceParams(pk, 16, False).new_ballot([1, 0, 1] + [0] * 12 + [1], r),
        "qv": lambda r: oq.new_ballot([4, 2, 0, 0, 0], r),
        "zero": k.encrypt_zero,
        "bool": lambda r: k.encrypt_bool(True, r),
        "range": lambda r: k.encrypt_range(pr, 42, r),
        "u64": lambda r: k.encrypt_u64(7, r),
        "sumsq": lambda r: b"".join(k.sumsq_snapshot([1, 2, 3], r)),
        "share": lambda r: o.decryption_share_new(E.sc(5), E.element(9), 3, 2, pk, 1, r),
    }
    for name, make in makers.items():
        plain = make(o.rng_from_u64(77))
        with o.Script() as s:
            assert make(o.rng_from_u64(77)) == plain, name
        assert s.trace, name
        with o.Script({("ring_response", 9, 9, 9): 1}):                    # a pin that matches no draw
            assert make(o.rng_from_u64(77)) == plain, name
    # the reference's snapshot batch is the same with a script in force
    assert op.generate_batch(12345, 0, 4, threads=1) == b"".join(
        op.new_ballot(o.select_single(12345 + i, 5), o.rng_from_u64(12345 + i)) for i in range(4))


def test_trace_names_every_draw_and_a_pin_moves_only_its_own_draw(oracle):
    o = oracle
    _, pk, _ = o.keypair_from_seed(12345)
    op = o.ChoiceParams(pk, 5, True)
    with o.Script() as s:
        a = op.new_ballot([0, 1, 0, 0, 0], o.rng_from_u64(3))
    roles = [t[0] for t in s.trace]
    assert roles.count("ct_r") == 5 and roles.count("ring_nonce") == 5 and roles.count("ring_response") == 5
    assert roles.count("logeq_nonce") == 1 and len(roles) == 16
    assert ("ring_response", 0, 1, 0) in s.trace and ("ring_response", 0, 0, 1) in s.trace
    oq = o.QvParams(pk, 5, 20)
    with o.Script() as q:
        oq.new_ballot([4, 2, 0, 0, 0], o.rng_from_u64(3))
    scopes = {t[1] for t in q.trace if t[0] in ("value_r", "ring_nonce")}
    assert scopes == set(range(6))                                      # 5 votes + the credit range proof
    assert sum(t[0] == "sumsq_er" for t in q.trace) == 5 and sum(t[0] == "sumsq_ez" for t in q.trace) == 1
    # pinning ring 2's free response changes that response (and what hashes it), not the draws after it
    with o.Script({("ring_response", 0, 2, 1): 12345}):
        b = op.new_ballot([0, 1, 0, 0, 0], o.rng_from_u64(3))
    resp = lambda x, j, kk: x[32 * (10 + 1 + 2 * j + kk) : 32 * (10 + 2 + 2 * j + kk)]      # noqa: E731
    assert resp(b, 2, 1) == E.sc(12345) != resp(a, 2, 1)
    assert resp(b, 3, 1) == resp(a, 3, 1) and resp(b, 4, 1) == resp(a, 4, 1)              # later free draws: the same stream
    assert b[:320] == a[:320]                                           # ciphertexts were drawn before it
    assert op.verify(b) == 0
