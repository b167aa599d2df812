"""The multi-scalar cases of tests/msm_cases.py without a GPU: the exact reference equals the oracle's point_multi_mul on small instances
of every mode, the recoding model gives every case scalar back, the layout model gives known values, and every GPU case of MATRIX
reaches the edge it is named for."""
import numpy as np
import pytest

import msm_cases as mc
from msm_cases import L, sc


@pytest.fixture(scope="module")
def pool():
    return mc.make_pool()


def _oracle_product(case, pool, with_r):
    keep = [t for t in range(case.terms) if t not in case.bad]
    ks = b"".join(bytes(case.scalars[t]) for t in keep)
    ps = b"".join(pool.encoding(int(case.idx[t])) for t in keep)
    got = mc.o.point_multi_mul(ks, ps) if keep else bytes(32)
    return mc.o.point_add(got, mc.o.point_mul_generator(sc(case.r))) if with_r else got


def _small(mode, c, pool, terms=None):
    """A small instance of a mode; the digit patterns are those of window width c (built from the forced size that gives c)."""
    terms = terms or {12: 96, 13: 160, 14: 256, 15: 384}[c]
    cases = mc.build(mode, terms, pool, 1000 + c)
    if mode == "digits":
        pats = mc._from_ints(mc.digit_patterns(c))
        for case in cases:
            case.scalars = pats[np.arange(terms) % len(pats)]
    return cases


@pytest.mark.parametrize("c", (12, 13, 14, 15))
@pytest.mark.parametrize("mode", mc.MODES)
def test_reference_equals_oracle(pool, mode, c):
    for case in _small(mode, c, pool):
        for with_r in (False, True):
            assert case.expected(pool, with_r) == _oracle_product(case, pool, with_r), (mode, c, with_r)
        if mode in ("zero", "pairs", "cancel"):
            assert case.expected(pool) == bytes(32)
            assert case.expected(pool, True) == mc.o.point_mul_generator(sc(case.r))


def test_reference_with_undecodable_points_skips_them(pool):
    (case,) = mc.build("bad", 64, pool, 5)
    assert case.bad == (0, 63)
    assert case.expected(pool) != mc.Case(case.scalars, case.idx).expected(pool)
    assert mc.o.point_multi_mul(bytes(case.scalars[0]), mc.UNDECODABLE) is None


def test_pool_layout(pool):
    h = pool.half
    assert len(pool) == mc.POOL_SIZE and pool.logs[0] == pool.logs[h] == 0
    assert pool.encoding(0) == mc.IDENTITY and pool.logs[1] == 1 and pool.logs[h + 1] == L - 1
    assert all((pool.logs[j] + pool.logs[h + j]) % L == 0 for j in range(h))
    assert len(set(pool.logs[3:h])) == h - 3


@pytest.mark.parametrize("c", (12, 13, 14, 15))
def test_recoding_gives_every_scalar_back(pool, c):
    B = 1 << (c - 1)
    for mode in mc.MODES:
        for case in _small(mode, c, pool):
            digits, carries = mc.recode(case.scalars, c)
            assert int(np.abs(digits).max()) <= B
            assert not carries[-1].any()
            for t, k in enumerate(case.scalar_ints()):
                assert sum(int(d) << (c * w) for w, d in enumerate(digits[:, t])) == k, (mode, c, t)
    for k in mc.digit_patterns(c) + [0, 1, L - 1, 2**252 - 1, 2**253 - 1]:
        d, _ = mc.recode(mc._from_ints([k]) if k < L else np.frombuffer(k.to_bytes(32, "little"), np.uint8).reshape(1, 32), c)
        assert sum(int(x) << (c * w) for w, x in enumerate(d[:, 0])) == k


def test_digit_patterns_reach_their_digits():
    for c in (12, 13, 14, 15):
        B, pats = 1 << (c - 1), mc.digit_patterns(c)
        assert all(0 < p < L for p in pats) and L - 1 in pats
        d, carries = mc.recode(mc._from_ints(pats[:3]), c)
        full = 252 // c                                      # windows below the clip at bit 252
        assert (d[:full, 0] == B).all()                      # top bucket in every window
        assert (d[:full, 1] < 0).all() and carries[:full, 1].all()
        assert d[0, 2] == -1 and (d[1:full, 2] == 0).all() and carries[:full, 2].all()


def test_layout_model_known_values():
    assert [mc.levels(n) for n in (4096, 20001, 1 << 19, (1 << 19) + 1, 1 << 22, 1 << 24)] == [2, 3, 3, 4, 4, 4]
    assert [mc.window_bits(n) for n in (4096, 1 << 17, (1 << 17) + 1, (1 << 18) + 1, (1 << 19) + 1, 1 << 20, 1 << 24)] == [12, 12, 13, 14, 15, 15, 15]
    assert [mc.windows(c) for c in (12, 13, 14, 15)] == [22, 20, 19, 18]
    assert mc.layout(1 << 20)["tiles"] == 288 and mc.layout(20001)["tiles"] == 44


def test_matrix_covers_the_issue():
    """Random and digit-pattern modes at c = 13, 14 and 15; every mode at c = 15 with 4 levels; the three entries on the c = 15 random and
    equal-scalar cases; the sizes around both switches and the documented maximum."""
    by = {}
    for s in mc.MATRIX:
        if mc.uses_buckets(s):
            by.setdefault(s.mode, set()).add((mc.window_bits(s.terms), mc.levels(s.terms)))
    assert set(mc.MODES) <= set(by)
    assert all((15, 4) in v for v in by.values())
    assert {13, 14, 15} <= {c for c, _ in by["random"]} and {13, 14, 15} <= {c for c, _ in by["digits"]}
    names = {s.name: s for s in mc.MATRIX}
    assert set(names["c15_random"].entries) == set(names["c15_equal"].entries) == {"host", "device", "prepared"}
    assert {s.terms for s in mc.MATRIX} >= {1 << 17, (1 << 17) + 1, (1 << 18) + 1, (1 << 19) + 1, (1 << 20) - 1, 1 << 20, (1 << 20) + 255,
                                            1 << 22, 1 << 24}


@pytest.mark.parametrize("spec", mc.MATRIX, ids=lambda s: s.name)
def test_gpu_case_reaches_its_edge(pool, spec):
    need = spec.need
    assert mc.uses_buckets(spec) == need.get("buckets", True)
    lay = mc.layout(spec.terms)
    for k in ("c", "levels", "tiles"):
        if k in need:
            assert lay[k] == need[k], (spec.name, k, lay)
    if not any(k in need for k in mc.DATA_KEYS):
        return
    cases = mc.build(spec.mode, spec.terms, pool, spec.seed)
    stats = [mc.bucket_stats(case.scalars, lay["c"]) for case in cases]
    if "high_bucket" in need:
        assert any(s["high_bucket"] for s in stats) == need["high_bucket"], stats
    if "min_bucket" in need:               # a bucket longer than levels - 1 rounds of pieces can cover: the last level does work
        assert max(s["max_bucket"] for s in stats) >= need["min_bucket"], stats
    if "min_carry_chain" in need:
        assert max(s["carry_chain"] for s in stats) >= need["min_carry_chain"], stats
    if "min_empty" in need:
        assert min(s["empty"] for s in stats) >= need["min_empty"], stats
    if need.get("log_zero"):
        assert all(case.log(pool) == 0 for case in cases)
    top = mc._from_ints([L - 1])[0]
    for case in cases:                     # canonical: below 2^252, or l - 1
        assert case.terms == spec.terms
        assert ((case.scalars[:, 31] < 0x10) | (case.scalars == top).all(axis=1)).all()
