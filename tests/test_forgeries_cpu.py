"""The forgery corpus (tests/forgery_cases.py) without a GPU, so that the GPU test cannot hide a failure behind a corpus that is not
what it says: the item layouts are right, the mutants are well formed (or malformed exactly where they say), the oracle accepts the
base objects and rejects EVERY forgery -- none is filtered out -- with the status words the constructions were made for, and every
status kind the engines can give on these elections is reached.

The oracle is the CPU restatement under oracle/ (and tests/commit_equiv_ref.py); no reference verifiers are built under oracle/_ref
(there is no toolchain for them), so the corpus is not run through them here."""
import collections
from math import isqrt

import pytest

import forgery_cases as F

CHALLENGE_KINDS = {"single": {4, 6}, "multi": {6}, "qv": {8, 10, 12}, "zero": {4}, "bool": {6}, "range": {6}, "share": {4}, "sumsq": {12},
                   "commit_equiv": {4}}


def _ids(fams):
    return [f"{n}-{k}" for n, k in fams]


@pytest.fixture(params=F.FAMILIES, ids=_ids(F.FAMILIES))
def fam(request, oracle):
    return F.family(*request.param)


def _verdicts(fam):
    return F.verdicts(fam.name, fam.key_name)


def test_layout_is_right_on_the_valid_base(oracle, fam):
    assert set(fam.layout) == {"P", "S"}
    assert len(fam.valid) >= 8 and len(set(fam.valid)) == len(fam.valid)
    for v in fam.valid + fam.extra.get("word_bases", []):
        assert len(v) == fam.size
        assert fam.well_formed(v)
        assert fam.verify(v) == oracle.OK
    if fam.kind == "range":                              # the product's decomposition against the oracle's
        assert F.range_rings(fam.credits) == [s for s, _ in fam.extra["range"].rings]
    if fam.kind == "qv":
        p = fam.oracle_params
        assert F.range_rings(isqrt(fam.credits) + 1) == [s for s, _ in p.vote_range.rings]
        assert F.range_rings(fam.credits + 1) == [s for s, _ in p.credit_range.rings]
        assert fam.size == p.ballot_size
    if fam.kind in ("single", "multi"):
        assert fam.size == fam.oracle_params.ballot_size


def test_mutants_are_well_formed_or_malformed_where_they_say(oracle, fam):
    blobs = [f.blob for f in fam.forgeries]
    assert len(set(blobs)) == len(blobs) and not set(blobs) & set(fam.valid)
    assert {f.mutation for f in fam.forgeries} >= {1, 2, 4, 6, 7}
    for f, st in zip(fam.forgeries, _verdicts(fam)):
        assert len(f.blob) == fam.size and f.family == fam.label and f.what_bug_it_catches
        if f.mutation == 1 or "_malformed_" in f.name:
            kind = oracle.BAD_POINT if fam.layout[f.item] == "P" else oracle.BAD_SCALAR
            assert st == oracle.status(kind, f.item), f.name
            assert not fam.well_formed(f.blob)
        else:
            assert fam.well_formed(f.blob), f.name
            assert st & 0xFF in CHALLENGE_KINDS[fam.kind], (f.name, st)


def test_the_oracle_rejects_every_forgery(oracle, fam):
    st = _verdicts(fam)
    assert len(st) == len(fam.forgeries) > 40
    assert [f.name for f, s in zip(fam.forgeries, st) if s == oracle.OK] == []
    if fam.tallies:                                      # the batch verifier and the one-ballot verifier agree
        assert [fam.verify(f.blob) for f in fam.forgeries[::7]] == list(st[::7])


def test_constructions_get_the_status_they_were_made_for(oracle, fam):
    o = oracle
    n = fam.n_options
    got = {f.name: s for f, s in zip(fam.forgeries, _verdicts(fam))}
    by = collections.defaultdict(list)
    for f, s in zip(fam.forgeries, _verdicts(fam)):
        by[f.mutation].append((f.name, s))
    want = {}
    if fam.kind == "single":
        # family 3: the sum proof holds, so the range proof alone rejects -- the point of the family
        assert len(by[3]) >= 6 * n and {s for _, s in by[3]} == {o.RANGE_CHALLENGE}, by[3]
        want = {"lie_two_ones": o.SUM_CHALLENGE, "lie_no_one": o.SUM_CHALLENGE, "lie_all_ones": o.SUM_CHALLENGE,
                "transplant_sum_proof": o.SUM_CHALLENGE, "transplant_ring_proof": o.RANGE_CHALLENGE,
                "two_sum_and_ring0": o.SUM_CHALLENGE, f"two_sum_and_ring{n - 1}": o.SUM_CHALLENGE, "two_sum_and_common_challenge": o.SUM_CHALLENGE}
        # every one-element mutation breaks the sum first
        assert {s for name, s in by[2] if int(name.split("@")[1]) < 2 * n} == {o.SUM_CHALLENGE}
    elif fam.kind == "qv":
        want = {"lie_credits_plus_1": o.QV_CREDIT_RANGE_CHALLENGE, "two_variant_and_credit_range": o.status(o.QV_VARIANT_CHALLENGE, n - 1),
                "two_credit_range_and_sumsq": o.QV_CREDIT_RANGE_CHALLENGE, "two_variant_and_sumsq": o.status(o.QV_VARIANT_CHALLENGE, 0),
                "transplant_sumsq_block": o.QV_CREDIT_EQUIV_CHALLENGE, f"transplant_block{n}": o.QV_CREDIT_EQUIV_CHALLENGE}
        want.update({f"lie_vote{i}_above_range": o.status(o.QV_VARIANT_CHALLENGE, i) for i in range(n)})
        # a vote block of another ballot proves its own range: only the sum of squares notices
        want.update({f"transplant_block{i}": o.QV_CREDIT_EQUIV_CHALLENGE for i in range(n)})
        two = [name for name, _ in by[7] if name.startswith("two_variants")]
        assert len(two) >= 2
        want.update({name: o.status(o.QV_VARIANT_CHALLENGE, int(name[len("two_variants"):].split("_")[0])) for name in two})
        assert any(name.startswith("made_for_qv") for name, _ in by[4])
    elif fam.kind == "range":
        want = {"lie_value_is_bound": o.RANGE_CHALLENGE}
        if fam.credits == 15:
            want["made_for_bound16"] = o.RANGE_CHALLENGE
    elif fam.kind == "share":
        want = {"made_for_index0": o.SUM_CHALLENGE, "made_for_index2": o.SUM_CHALLENGE}
    elif fam.kind == "commit_equiv":
        want = {"other_label_last_byte": o.SUM_CHALLENGE, "other_label_first_byte": o.SUM_CHALLENGE}
    want["other_key"] = min(CHALLENGE_KINDS[fam.kind]) if fam.kind != "qv" else o.status(o.QV_VARIANT_CHALLENGE, 0)
    for name, st in want.items():
        assert got[name] == st, (name, got[name], st)


def test_one_word_challenges(oracle, fam):
    """Family 8: each mutant differs from its accepted base in one 32-bit word of one challenge, and is rejected for that proof."""
    bases = fam.extra.get("word_bases", [])
    assert bool(bases) == (fam.kind != "share")
    words = [(f, s) for f, s in zip(fam.forgeries, _verdicts(fam)) if f.mutation == 8]
    assert len(words) == (48 if fam.kind == "qv" else 8 if bases else 0)
    for f, st in words:
        diff = [w for w in range(fam.size // 4) if f.blob[4 * w : 4 * w + 4] != bases[0][4 * w : 4 * w + 4]]
        item = int(f.name.split("@")[1])
        assert diff == [8 * item + int(f.name[4])], f.name
        assert st & 0xFF in CHALLENGE_KINDS[fam.kind]
    if fam.kind == "qv":                                 # one set of eight for every vote, the credit range and the sum of squares
        assert collections.Counter(s for _, s in words) == collections.Counter(
            {**{oracle.status(oracle.QV_VARIANT_CHALLENGE, i): 8 for i in range(fam.n_options)},
             oracle.QV_CREDIT_RANGE_CHALLENGE: 8, oracle.QV_CREDIT_EQUIV_CHALLENGE: 8})


def test_true_proofs_under_a_label_one_byte_away(oracle):
    for name in ("sumsq2", "commit_equiv"):
        fam = F.family(name)
        for label in F.OTHER_LABELS:
            other = fam.with_label(label)
            assert sum(a != b for a, b in zip(label, F.LABEL)) == 1
            assert {other.verify(v) for v in fam.valid} == {min(CHALLENGE_KINDS[fam.kind])}


def test_status_kinds_reached(oracle):
    o = oracle
    kinds = collections.defaultdict(set)
    for name, key in F.FAMILIES:
        kinds[F.family(name, key).kind] |= set(F.verdicts(name, key))
    everything = set().union(*kinds.values())
    assert {o.BAD_SCALAR, o.BAD_POINT} <= {s & 0xFF for s in everything}
    assert o.SUM_CHALLENGE in kinds["single"]
    assert o.RANGE_CHALLENGE in kinds["single"] and o.RANGE_CHALLENGE in kinds["multi"]
    qv = F.family("qv4x12")
    assert {o.status(o.QV_VARIANT_CHALLENGE, i) for i in range(qv.n_options)} <= kinds["qv"]
    assert {o.QV_CREDIT_RANGE_CHALLENGE, o.QV_CREDIT_EQUIV_CHALLENGE} <= kinds["qv"]
    assert o.OK not in everything
