"""The shuffle verifier's chain rows at the edges, without a GPU (tests/shuffle_edge_cases.py has the cases and says how they are made):
* the trapdoor builder against the model with the oracle judging: every built row passes CHAIN, every s^ + 1 fails it, every second
  s' + 1 fails exactly there; the placement puts every kind of scalar and point on every row at a tile's edge;
* the stated expectations of tampered proofs (expect_*), which the GPU tests rest on, against the same judge;
* the lanes of tests/hostcheck/shufflecheck.cpp (shuffle_kernels.cuh under -DEG_BOUNDCHECK with ASan + UBSan) on the edge cases;
* the chain kernel's grid at the sizes where its wavefronts take a second tile."""
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

import shuffle_cases as SC
import shuffle_edge_cases as E
import shuffle_ref as M
from test_shuffle_cpu import check, run_verify  # noqa: F401  (the host-check program and its verify subcommand)

JUDGES = max(1, min(8, os.cpu_count() or 1))
N = 190                                     # three tiles of 63 rows and one row
CASES, STEP = 53, 157                       # case k starts at row k STEP of the product list (test_placement says what that covers)
H_RANDOM = 0x0A5B1C6D2E7F3A4B5C6D7E8F9A0B1C2D3E4F5A6B7C8D9E0F1A2B3C4D5E6F7A % M.L
LANES_N = 67                                # the host-check lanes under the sanitizers: one tile and four rows


@pytest.fixture(scope="module")
def be(oracle):
    return M.OracleBackend()


@pytest.fixture(scope="module")
def K(be):
    return be.mul_generator([0xC0FFEE])[0]


def h_of(k):
    """H_0 = G in the even cases, [h]G with a fixed random h in the odd ones"""
    return 1 if k % 2 == 0 else H_RANDOM


def edge_case(be, K, k):
    return E.build(be, E.window(E.product_specs(), N, k * STEP), h_of(k), K, seed=7000 + k, name=f"edges_{k}")


def off_by_one_twins(t):
    """(all s^ + 1, every second s' + 1 where the predecessor is not the identity, those rows)"""
    n = len(t["ins"])
    rows = [i for i in range(n) if i % 2 == 1 and t["alpha_prev"][i] != 0]
    return E.with_rows(t, "shat_plus_one", "shat", range(n)), E.with_rows(t, "sprime_plus_one", "sprime", rows), rows


def check_case(be, t, run):
    """what every built case must satisfy, for a runner `run` (the judge itself, the host-check lanes or the device) that gives
    (verdict, rows, found); the model's answers are returned for the callers that compare another runner with them"""
    n = len(t["ins"])
    a, b, rows_b = off_by_one_twins(t)
    want = [SC.judge(be, E.twin_of(t)), SC.judge(be, a), SC.judge(be, b)]
    got = want if run is None else [run(E.twin_of(t)), run(a), run(b)]
    assert got == want, t["name"]
    mask, rows, found = got[0]
    assert not mask & (M.BAD_ENCODING | M.CHAIN) and rows == [0] * n and found == E.NONE4, t["name"]
    assert got[1][1:] == ([M.ROW_CHAIN] * n, [0, n, M.NONE, 0]) and got[1][0] & M.CHAIN and not got[1][0] & M.BAD_ENCODING, t["name"]
    assert got[2][1:] == E.expect_chain_rows(n, rows_b) and got[2][0] & M.CHAIN and not got[2][0] & M.BAD_ENCODING, t["name"]
    assert len(rows_b) >= n // 3
    return want


# ------------------------------------------------------------------ the builder and the placement
def test_lists():
    P = E.product_specs()
    real = [s for s in P if s["edge"] is not None]
    assert len(P) == 960 and len({(s["t"], s["edge"], s["role"], s["c"]) for s in real}) == 3 * 20 * 2 * 7 == len(real)
    assert len(set(E.EDGES.values())) == 20 and all(0 <= v < M.L for v in E.EDGES.values())
    digits = lambda v: [(v >> (4 * i)) & 15 for i in range(64)]
    assert digits(E.EIGHTS) == [8] * 63 + [0] and digits(E.SEVENS) == [7] * 63 + [0] and digits(E.EDGES["2^252-1"]) == [15] * 63 + [0]
    C = E.cover_specs()
    assert {(s["edge"], s["role"]) for s in C if s["edge"] is not None} == {(e, r) for e in E.EDGES for r in E.ROLES}
    assert {s["c"] for s in C} == set(E.C_KINDS) and {s["t"] for s in C} == set(E.T_KINDS) and len(C) <= LANES_N


def test_placement():
    """N is no multiple of 63, and over the cases every scalar edge in either role, every kind of c^ and every kind of t^ stands on
    EVERY one of the rows 0, 61, 62, 63, 64, 125, 126 and N - 1; row 0 sees H_0 = G and H_0 = [h]G"""
    assert N % 63 and E.edge_rows(N) == [0, 61, 62, 63, 64, 125, 126, N - 1]
    P = E.product_specs()
    for row in E.edge_rows(N):
        at = [E.window(P, N, k * STEP)[row] for k in range(CASES)]
        at = [s for s in at if s["edge"] is not None]
        assert {(s["edge"], s["role"]) for s in at} == {(e, r) for e in E.EDGES for r in E.ROLES}, row
        assert {s["c"] for s in at} == set(E.C_KINDS) and {s["t"] for s in at} == set(E.T_KINDS), row
    assert {h_of(k) for k in range(CASES)} == {1, H_RANDOM}


def test_built_rows_pass_and_their_neighbours_in_value_fail(be, K):
    """every case: judged by the oracle, no row fails, nothing is badly encoded (the T bits fail: head, c, in and out are arbitrary);
    s^ + 1 in every row fails every row; s' + 1 in every second row fails exactly those"""
    with ThreadPoolExecutor(JUDGES) as pool:
        cases = list(pool.map(lambda k: edge_case(be, K, k), range(CASES)))
        wants = list(pool.map(lambda t: check_case(be, t, None), cases))
    # the model agrees with the integers the builder solved: tau = -x a + s^ + s' a_prev in every row
    t = cases[1]
    assert t["alpha_prev"][0] == H_RANDOM and cases[0]["alpha_prev"][0] == 1
    assert all(w[0][0] == M.T1 | M.T2 | M.T3 | M.T41 | M.T42 for w in wants)
    # the row with both scalars zero (c^ and t^ the identity) is among them, and rows whose sum is the identity
    both_zero = sum(1 for c in cases for i in range(N) if c["shat"][i] == 0 and c["sprime"][i] == 0)
    assert both_zero >= 1 and sum(1 for c in cases for s in c["specs"] if s["t"] == "identity") > 100


def test_the_builder_refuses_what_cannot_be_solved(be, K):
    with pytest.raises(ValueError):
        E.build(be, [{"c": "identity", "t": "random", "role": "sprime", "edge": "1"}, {"c": "random", "t": "G", "role": "shat", "edge": "1"}], 1, K, 1)


# ------------------------------------------------------------------ the stated expectations of tampered proofs
@pytest.fixture(scope="module")
def key(be):
    return M.derive_key(be, SC.SEED, N)


def judged(be, twins):
    with ThreadPoolExecutor(JUDGES) as pool:
        return list(pool.map(lambda t: SC.judge(be, t), twins))


@pytest.mark.parametrize("n,every", [(7, True), (64, True), (N, False)])
def test_expectations_hold_against_the_judge(be, K, key, n, every):
    """expect_shat_plus_one, expect_scalar_is_l and expect_chat_not_a_point at every row of the small sizes; at N = 190 (a judgement of
    every row there is 190 runs of the model) at the tiles' edges, at seeded random rows and for the sets of rows the GPU test uses"""
    import random

    c = M.make(be, K, key, SC.PREFIX, n, 31000 + n)
    base = SC.base(c, K, key)
    assert SC.judge(be, base) == (0, [0] * n, E.NONE4)
    ks = list(range(n)) if every else sorted(set(E.edge_rows(n)) | set(random.Random(5).sample(range(n), 8)))
    twins, want = [], []
    for k in ks:
        twins.append(E.with_rows(base, f"shat_plus_one_{k}", "shat", [k]))
        want.append(E.expect_shat_plus_one(n, [k]))
        assert want[-1] == (M.CHAIN, [M.ROW_CHAIN if i == k else 0 for i in range(n)], [0, 1, M.NONE, k])
    for k in E.edge_rows(n):
        for sec in ("sprime", "shat"):
            twins.append(E.with_rows(base, f"{sec}_is_l_{k}", sec, [k], E.LL))
            want.append(E.expect_scalar_is_l(n, k))
        twins.append(E.with_rows(base, f"chat_not_a_point_{k}", "chat", [k], SC.NOT_A_POINT))
        want.append(E.expect_chat_not_a_point(n, k))
        if k + 1 < n:
            assert want[-1][1][k:k + 2] == [M.ROW_BAD, 0]
    for name, rows in row_sets(n).items():
        twins.append(E.with_rows(base, name, "shat", rows))
        want.append(E.expect_shat_plus_one(n, rows))
    got = judged(be, twins)
    for t, g, w in zip(twins, got, want):
        assert g == w, (n, t["name"])


def row_sets(n):
    """the sets of rows that fail together: the last lane of every tile, the first lane of every tile"""
    return {"ends_of_tiles": [i for i in range(n) if i % 63 == 62], "starts_of_tiles": [i for i in range(n) if i % 63 == 0]}


def test_expectation_functions_on_their_own():
    assert E.expect_shat_plus_one(5, []) == (0, [0] * 5, E.NONE4)
    assert E.expect_shat_plus_one(5, [3, 1], M.T2) == (M.T2 | M.CHAIN, [0, 2, 0, 2, 0], [0, 2, M.NONE, 1])
    assert E.expect_chat_not_a_point(3, 2) == (M.BAD_ENCODING, [2, 2, 1], [1, 2, 2, 0])
    assert E.expect_chat_not_a_point(1, 0) == (M.BAD_ENCODING, [1], [1, 0, 0, M.NONE])
    assert E.expect_chat_not_a_point(3, 0) == (M.BAD_ENCODING, [1, 0, 2], [1, 1, 0, 2])


# ------------------------------------------------------------------ the host-check lanes on the edge cases
def lanes_case(be, K, k):
    """the short list at N = 67, from its row 3 on, and from row 26 on in the second case: every scalar edge in either role and every kind of point in
    both, and rows 62 / 63 (the last lane of a tile, the first of the next) hold an edge each time"""
    return E.build(be, E.window(E.cover_specs(), LANES_N, 3 + 23 * k), h_of(k), K, seed=7100 + k, name=f"lanes_{k}")


def test_lane_cases_keep_every_kind(be, K):
    for k in (0, 1):
        specs = E.window(E.cover_specs(), LANES_N, 3 + 23 * k)
        assert {(s["edge"], s["role"]) for s in specs if s["edge"] is not None} == {(e, r) for e in E.EDGES for r in E.ROLES}
        assert {s["c"] for s in specs} == set(E.C_KINDS) and {s["t"] for s in specs} == set(E.T_KINDS)
        assert specs[62]["edge"] is not None and specs[63]["edge"] is not None and LANES_N % 63


def test_the_lanes_pass_the_edge_rows(check, be, K, tmp_path):  # noqa: F811
    """the lane functions in the kernels' arrangement: the built rows pass, the off-by-one twins fail where they must, and all of it is
    the model's word for word"""
    cases = [lanes_case(be, K, k) for k in (0, 1)]
    runs = []
    for t in cases:
        a, b, _ = off_by_one_twins(t)
        runs += [E.twin_of(t), a, b]
    with ThreadPoolExecutor(JUDGES) as pool:
        got = list(pool.map(lambda kt: run_verify(check, tmp_path, kt[1], f"_edge{kt[0]}"), enumerate(runs)))
    for i, t in enumerate(cases):
        answers = iter(got[3 * i:3 * i + 3])
        check_case(be, t, lambda _twin: next(answers))


# ------------------------------------------------------------------ the chain kernel's grid where a wavefront takes a second tile
@pytest.mark.parametrize("cus", [64, 256, 304])
def test_second_pass_size(check, cus):  # noqa: F811
    n = second_pass_rows(cus)
    total, grid = map(int, check("layout", n, cus, 0, 0, 0).split("\n")[0].split())
    tiles = -(-n // 63)
    assert grid == 4 * cus and tiles == 4 * grid + 2 and n % 63 == 5                # one full tile and one of five rows beyond the first pass


def second_pass_rows(cus):
    """the rows of 16 wavefronts on every CU, one more tile and five rows"""
    return 63 * 16 * cus + 63 + 5
