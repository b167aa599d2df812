"""The HIP verify path on VALID ballots built from edge-case randomness (tests/edge_ballots.py): identity commitments and
ciphertexts, sums over the identity, responses on the comb-digit corners, tallies that cancel.  On these the kernels' edge handling
decides an honest voter's verdict and the tally, so every verdict must be 0 and equal the oracle's, and every tally the oracle's.
Each case is checked by the oracle's counters first (test_edge_ballots_cpu.py), so none passes vacuously."""
import json
import random

import pytest

import edge_ballots as E

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


def _edges(fam):
    return [e.ballot for e in fam.edges]


def _with_twins(fam):
    """edge ballots interleaved with their tampered twins (the challenge flipped; a random bit flipped)."""
    out = []
    for i, e in enumerate(fam.edges):
        out += [e.ballot, E.tamper(e.ballot, i, fam.challenge_item), E.tamper(e.ballot, 1000 + i)]
    return out


def _check(fam, params, ballots, accept=None):
    """verdicts (and the tally) of the HIP path == the oracle's; `accept` = indices that must be accepted."""
    want = [fam.verify(b) for b in ballots]
    for i in accept if accept is not None else range(len(ballots)):
        assert want[i] == 0, i
    raw = b"".join(ballots)
    if fam.tallies:
        got, tally = params.verify_batch(raw)
        assert got == want
        assert tally == fam.tally(raw, want)
        return want, tally
    assert params.verify_batch(raw) == want
    return want, None


@pytest.mark.parametrize("fam_name", E.FAMILY_NAMES)
def test_edge_corpus_verdicts_and_tallies(eg, ctx, fam_name):
    """Every family under every key (golden, G, -G, [2]G) on the default engine: edge ballots accepted, tampered twins get the
    oracle's status words, the tally is the oracle's; for elections, a batch of the cancelling pair tallies to the identity."""
    for key_name in E.KEY_NAMES:
        fam = E.family(fam_name, key_name)
        p = fam.gpu_params(eg, ctx)
        try:
            batch = _with_twins(fam)
            want, _ = _check(fam, p, batch, accept=range(0, len(batch), 3))
            assert all(w != 0 for w in want[1::3]), key_name
            if fam.tallies:
                pair = [e.ballot for e in fam.edges if e.name.startswith("cancel_")]
                _, tally = _check(fam, p, pair + [E.tamper(pair[0], 5, fam.challenge_item)], accept=[0, 1])
                assert all(tally[64 * k : 64 * k + 32] == E.IDENTITY for k in range(fam.n_options))
                assert any(tally[64 * k + 32 : 64 * k + 64] == E.IDENTITY for k in range(fam.n_options))
        finally:
            p.close()


@pytest.mark.parametrize("fam_name", ["single5", "multi20", "qv5x20"])
def test_edge_ballots_placed_among_random_ones(eg, ctx, fam_name, monkeypatch):
    """Edge ballots at lanes 0, 63, 64 and the last lane, one whole wavefront of them, the rest ordinary ballots (uniform
    randomness), some of them tampered; then the same with a small EG_CHUNK so that edge ballots sit on both sides of chunk
    boundaries."""
    fam = E.family(fam_name)
    edges = _edges(fam)
    rnd = random.Random(fam_name)
    n = 320
    rand = fam.random_ballots(4711, n)
    batch = [rand[i * fam.size : (i + 1) * fam.size] for i in range(n)]
    for i in range(3, n, 17):
        batch[i] = E.tamper(batch[i], i)
    slots = [0, 63, 64, n - 1] + list(range(128, 192)) + [255, 256, 257]
    for j, s in enumerate(slots):
        batch[s] = edges[j % len(edges)] if j else [e.ballot for e in fam.edges if e.needs][0]
    for k in range(8):                                   # and scattered
        batch[rnd.randrange(n)] = rnd.choice(edges)
    accept = [i for i, b in enumerate(batch) if b in set(edges)]
    for chunk in (None, "128"):
        if chunk:
            monkeypatch.setenv("EG_CHUNK", chunk)        # read when the params object is made
        p = fam.gpu_params(eg, ctx)
        try:
            _check(fam, p, batch, accept)
        finally:
            p.close()


@pytest.mark.parametrize("big_bits", [24, 0])
def test_edge_corpus_on_wide_combs(eg, monkeypatch, big_bits):
    """Wide fixed-base combs forced from the first ballot (EG_COMB_BIG_MIN=1; 24-bit windows, and switched off): the corner
    responses of both widths through k_eq_table, for the golden key and -G, one context per key (the wide tables of G and K take
    some 11 GB each)."""
    monkeypatch.setenv("EG_COMB_BIG_MIN", "1")
    monkeypatch.setenv("EG_COMB_BIG_BITS", str(big_bits))
    for key_name in ("golden", "-G"):
        c = eg.Context(0)
        try:
            for name in ("single2", "single5", "qv5x20"):
                fam = E.family(name, key_name)
                p = fam.gpu_params(eg, c)
                try:
                    _check(fam, p, _with_twins(fam), accept=range(0, 3 * len(fam.edges), 3))
                finally:
                    p.close()
            assert c.comb_table_bits() == (20, big_bits)
        finally:
            c.close()


@pytest.mark.parametrize("group", ["1", "2"])
def test_edge_corpus_on_the_ring_group_walk(eg, ctx, monkeypatch, group):
    """The ring-group walk (EG_RING_GROUP rings per group: the sum tables accumulated group by group) on the edge ballots,
    whose sum bases cancel or are the identity."""
    monkeypatch.setenv("EG_RING_GROUP", group)
    for name in ("single5", "single16", "multi20"):
        for key_name in ("golden", "2G"):
            fam = E.family(name, key_name)
            assert eg.plan_describe(fam.kind, fam.n_options)["ring_group"] == int(group)
            p = fam.gpu_params(eg, ctx)
            try:
                _check(fam, p, _with_twins(fam), accept=range(0, 3 * len(fam.edges), 3))
            finally:
                p.close()


@pytest.mark.parametrize("fam_name", ["single5", "multi3of16", "qv5x20"])
def test_edge_corpus_through_the_other_entries(eg, ctx, fam_name):
    """The device-pointer entry, the host-buffer entry on raw pointers and verify_json on the same ballots as JSON text."""
    import torch
    from elastic_elgamal_amd import ingest, serde

    fam = E.family(fam_name)
    batch = _with_twins(fam)
    raw = b"".join(batch)
    n = len(batch)
    want = [fam.verify(b) for b in batch]
    want_tally = fam.tally(raw, want)
    assert want[::3] == [0] * len(fam.edges)
    p = fam.gpu_params(eg, ctx)
    try:
        d = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
        st = torch.full((n,), 99, dtype=torch.int32, device="cuda")
        p.tally_reset()
        p.verify_batch_device(n, d.data_ptr(), st.data_ptr())
        ctx.synchronize()
        assert [int(v) & 0xFFFFFFFF for v in st.cpu().tolist()] == want
        assert p.tally_encode() == want_tally
        hb = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
        hs = torch.zeros(n, dtype=torch.int32).pin_memory()
        tb = torch.zeros(64 * fam.n_options, dtype=torch.uint8)
        p.verify_batch_host_ptr(n, hb.data_ptr(), hs.data_ptr(), tb.data_ptr())
        assert [int(v) & 0xFFFFFFFF for v in hs.tolist()] == want and bytes(tb.numpy().tobytes()) == want_tally
        if fam.kind == "qv":
            objs = [ingest.unpack_qv_ballot(b, fam.n_options, fam.credits) for b in batch]
        else:
            objs = [serde.unpack_encrypted_choice(b, fam.n_options, fam.kind == "single") for b in batch]
        p.tally_reset()
        jgot, jtally = p.verify_json(json.dumps(objs))
        assert jgot == want and jtally == want_tally
    finally:
        p.close()


@pytest.mark.parametrize("fam_name", ["single5", "qv5x20"])
def test_edge_corpus_on_the_multi_device_entry(eg, ctx, fam_name):
    """Two contexts stand in for two GPUs; the second slab holds the cancelling pair as its only accepted ballots, so its tally is
    the identity in R of every slot (and in B of the slots not chosen), and the merged tally is the first slab's plus that."""
    fam = E.family(fam_name, "-G")
    pair = [e.ballot for e in fam.edges if e.name.startswith("cancel_")]
    first = _with_twins(fam)
    first = [b for b in first if b not in pair]
    other = eg.Context(0)
    objs = [fam.gpu_params(eg, ctx), fam.gpu_params(eg, other)]
    try:
        sizes = (len(first), len(pair))
        # verify_batch_multi splits evenly: hand it slabs of the same size by padding the pair's side with tampered copies
        pad = [E.tamper(pair[0], 7 + i, fam.challenge_item) for i in range(sizes[0] - sizes[1])]
        batch = first + pad + pair
        raw = b"".join(batch)
        want = [fam.verify(b) for b in batch]
        for o in objs:
            o.tally_reset()
        st, t = eg.verify_batch_multi(objs, raw)
        assert want[-2:] == [0, 0] and want[: len(first) : 3].count(0) >= len(first) // 3 - 1
        assert st == want and t == fam.tally(raw, want)
        second = objs[1].tally_encode()
        assert second == fam.tally(b"".join(pad + pair), want[len(first) :])
        assert all(second[64 * k : 64 * k + 32] == E.IDENTITY for k in range(fam.n_options))
        assert any(second[64 * k + 32 : 64 * k + 64] == E.IDENTITY for k in range(fam.n_options))
        assert objs[0].tally_encode() == fam.tally(b"".join(first), want[: len(first)])
        assert t == eg.tally_encode_multi(objs)
    finally:
        for o in objs:
            o.close()
        other.close()


def test_edge_scalars_through_the_primitive_tier(eg, ctx, oracle):
    """vartime_double_mul_generator and vartime_multi_mul with the corner scalars over +-G, [2]G and the identity, including
    products that cancel to the identity."""
    grp = eg.Ristretto(ctx)
    L = E.L
    pts = [E.element(1), E.element(L - 1), E.element(2), E.IDENTITY]
    cs = list(E.corner_scalars())
    ks, ps, rs, cancel = [], [], [], []
    for i, c in enumerate(cs):
        p = pts[i % 4]
        ks.append(E.sc(c)); ps.append(p); rs.append(E.sc(cs[(i * 7) % len(cs)]))
        # [c](-G) + [c]G and [c]([2]G) + [-2c]G cancel
        ks.append(E.sc(c)); ps.append(pts[1]); rs.append(E.sc(c)); cancel.append(len(ks) - 1)
        ks.append(E.sc(c)); ps.append(pts[2]); rs.append(E.sc(-2 * c)); cancel.append(len(ks) - 1)
    out, ok = grp.vartime_double_mul_generator(b"".join(ks), b"".join(ps), b"".join(rs))
    assert set(ok) == {1}
    for i in range(len(ks)):
        assert out[32 * i : 32 * i + 32] == oracle.point_double_mul_generator(ks[i], ps[i], rs[i]), i
    assert all(out[32 * i : 32 * i + 32] == E.IDENTITY for i in cancel)
    # three-term products over (G, -G, [2]G) and the identity: [a]G + [b](-G) + [c][2]G, cancelling when b = a + 2c
    terms, sk, sp, zero = 4, [], [], []
    for i, a in enumerate(cs):
        c = cs[(3 * i + 1) % len(cs)]
        b = (a + 2 * c) % L if i % 2 == 0 else cs[(5 * i + 2) % len(cs)]
        sk += [E.sc(a), E.sc(b), E.sc(c), E.sc(cs[(i + 9) % len(cs)])]
        sp += [pts[0], pts[1], pts[2], pts[3]]
        if i % 2 == 0:
            zero.append(i)
    out, ok = grp.vartime_multi_mul(terms, b"".join(sk), b"".join(sp))
    assert set(ok) == {1}
    for i in range(len(cs)):
        want = oracle.point_multi_mul(b"".join(sk[terms * i : terms * i + terms]), b"".join(sp[terms * i : terms * i + terms]))
        assert out[32 * i : 32 * i + 32] == want, i
    assert all(out[32 * i : 32 * i + 32] == E.IDENTITY for i in zero)
