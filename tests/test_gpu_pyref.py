"""The HIP verifiers against the verdicts of tests/pyref, the pure-Python verifier written from the reference's Rust source.  Nothing
is verified in Python here: the committed fixture (tests/golden/pyref_verdicts.json: pyref's status word of every case of
tests/pyref_cases.py, a SHA-256 prefix of every case and one SHA-256 over every family's bytes, the SHA-256 of pyref's tally of every election)
is the judge.  tests/test_pyref_cpu.py regenerates that fixture and compares it with the C oracle; here the oracle judges nothing.

Sweep items are made by the HIP provers from the module's seeds, edge and forgery items as tests/test_gpu_edge_ballots.py and
tests/test_gpu_forgeries.py build them.  Every item is hashed; an item whose hash the fixture does not hold FAILS the test.  Every
family runs as one batch with its twins interleaved, so accepted and rejected items share wavefronts, and once more reversed, so
every item meets both lane phases of the two-ballots-a-lane tail (a lane holds the ballots j and j + ceil(n / 2)); through the
host batch entry, the device-pointer entry and, for ballots, both `_small` entries."""
import hashlib
import json

import pytest

import pyref_cases as PC

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


def _fixture_words(jf, cases):
    """The fixture's status word of every case, looked up by the hash of its bytes."""
    known = PC.fixture_words(jf.id)
    missing = [c.name for c in cases if c.sha[:8] not in known]
    assert not missing, f"{jf.id}: bytes the fixture does not hold (the prover's bytes changed, or the fixture is stale): {missing[:8]}"
    return [known[c.sha[:8]] for c in cases]


def _device_words(ctx, n, raw, call):
    import torch

    d = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    st = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    call(n, d.data_ptr(), st.data_ptr())
    ctx.synchronize()
    return [int(v) & 0xFFFFFFFF for v in st.cpu().tolist()]


def _check(ctx, jf, params, cases):
    """Status words (and the tally) of every entry that applies == the fixture's, for `cases` in this order."""
    want = _fixture_words(jf, cases)
    assert want.count(0) >= sum(c.valid for c in cases) > 0
    raw = b"".join(c.blob for c in cases)
    n = len(cases)

    def same(got, entry):
        wrong = [(cases[i].name, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not wrong and len(got) == n, f"{jf.id} {entry} (case, HIP, pyref): {wrong[:10]}"

    if not jf.fam.tallies:
        same(params.verify_batch(raw), "eg_verify_proof_batch")
        same(_device_words(ctx, n, raw, params.verify_device), "eg_verify_proof_batch_device")
        return
    # every case of the family sits in the batch once, so the batch's tally is the fixture's tally of the accepted cases
    tally = PC.load_fixture()["families"][jf.id]["tally_sha256"]
    assert len(cases) == len(jf.cases)
    for entry in ("verify_batch", "verify_small"):
        got, got_tally = getattr(params, entry)(raw)
        same(got, entry)
        assert hashlib.sha256(got_tally).hexdigest() == tally, (jf.id, entry)
    for entry in ("verify_batch_device", "verify_small_device"):
        params.tally_reset()
        same(_device_words(ctx, n, raw, getattr(params, entry)), entry)
        assert hashlib.sha256(params.tally_encode()).hexdigest() == tally, (jf.id, entry)


def _both_orders(ctx, jf, params):
    # the lookup key is a prefix of a case's SHA-256; the family's digest over the full SHA-256 of every case binds every byte
    assert PC.family_digest(jf.cases) == PC.load_fixture()["families"][jf.id]["digest"], f"{jf.id}: bytes the fixture does not hold"
    _check(ctx, jf, params, jf.cases)
    _check(ctx, jf, params, jf.cases[::-1])


@pytest.mark.parametrize("name", PC.SWEEP_NAMES)
def test_shape_sweep_from_the_hip_prover(eg, ctx, name):
    jf, params = PC.sweep_family_gpu(name, eg, ctx)
    try:
        _both_orders(ctx, jf, params)
    finally:
        params.close()


@pytest.mark.parametrize("name", PC.E.FAMILY_NAMES)
def test_edge_corpus(eg, ctx, name):
    jf = PC.edge_family(name)
    params = jf.fam.gpu_params(eg, ctx)
    try:
        _both_orders(ctx, jf, params)
    finally:
        params.close()


@pytest.mark.parametrize("name,key_name", PC.F.FAMILIES, ids=[f"{n}-{k}" for n, k in PC.F.FAMILIES])
def test_forgery_corpus(eg, ctx, name, key_name):
    jf = PC.forgery_family(name, key_name)
    params = jf.fam.gpu_params(eg, ctx)
    try:
        _both_orders(ctx, jf, params)
    finally:
        params.close()


@pytest.mark.parametrize("name", PC.OBJECT_NAMES)
def test_objects_of_another_shape_through_verify_json(eg, ctx, name):
    """The *_LEN verdicts: objects whose shape is not the election's, as JSON text through the native entry (the library's object
    path resolves them)."""
    jf = PC.object_family(name)
    assert PC.family_digest(jf.cases) == PC.load_fixture()["families"][jf.id]["digest"]
    want = _fixture_words(jf, jf.cases)
    assert {w & 0xFF for w in want} - {0} >= ({3, 5} if jf.fam.kind == "single" else {3, 7, 9, 11})
    params = jf.fam.gpu_params(eg, ctx)
    try:
        for cases, words in ((jf.cases, want), (jf.cases[::-1], want[::-1])):
            got, _ = params.verify_json(b"[" + b",".join(c.blob for c in cases) + b"]")
            assert got == words, [(c.name, hex(g), hex(w)) for c, g, w in zip(cases, got, words) if g != w]
    finally:
        params.close()


def test_an_unknown_hash_fails():
    """The rule itself: bytes the fixture does not hold are an error, never a skip."""
    jf = PC.edge_family("zero")
    other = PC.Case("not in the fixture", bytes(jf.fam.size))
    with pytest.raises(AssertionError, match="does not hold"):
        _fixture_words(jf, [jf.cases[0], other])
    assert json.loads(PC.FIXTURE.read_text())["families"][jf.id]["sha8"][:8] == jf.cases[0].sha[:8]
    changed = [PC.Case(jf.cases[0].name, jf.cases[0].blob[:-1] + b"\0")] + jf.cases[1:]
    assert PC.family_digest(changed) != PC.load_fixture()["families"][jf.id]["digest"]
