"""The bounded discrete-log solver on the GPU (eg_dlog_solver_*, csrc/dlog_kernels.cuh) against the parent's table
(eg_dlog_table_*), against elements made by the oracle, and through the tally it exists for.  Exact everywhere: integer work."""
import ctypes as C
import random
import threading
import time

import pytest

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493
P = 2**255 - 19
TOP = 2**64 - 1
RUN = 64          # giant steps per lane (csrc/dlog_host.hpp)
ZERO = b"\0" * 32


def sc(x):
    return (x % L).to_bytes(32, "little")


@pytest.fixture(scope="module")
def eg():
    import elastic_elgamal_amd as m

    return m


@pytest.fixture(scope="module")
def T():
    from elastic_elgamal_amd import tally

    return tally


@pytest.fixture(scope="module")
def ctx(eg):
    c = eg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grp(eg, ctx):
    return eg.Ristretto(ctx)


@pytest.fixture(scope="module")
def small(T, grp):
    """Solvers with 2^8 and 2^10 baby entries: giant steps, run seams and lane seams occur on small data."""
    s = {bits: T.DiscreteLogSolver(grp, bits) for bits in (8, 10)}
    yield s
    for v in s.values():
        v.close()


@pytest.fixture(scope="module")
def default_solver(T, grp):
    s = T.DiscreteLogSolver(grp)
    yield s
    s.close()


@pytest.fixture(scope="module")
def multiples(grp):
    """[m]G for m in [0, 6100), made once by the GPU primitive (the same products the parent's table is made of)."""
    n = 6100
    raw = grp.mul_generator(b"".join(sc(m) for m in range(n)))
    return [raw[32 * m : 32 * m + 32] for m in range(n)]


def table_get(eg, table, elements):
    n = len(elements)
    values, found = (C.c_uint64 * n)(), C.create_string_buffer(n)
    eg._check(eg._load().eg_dlog_table_get(table._h, n, b"".join(elements), values, found))
    return [int(values[i]) if found.raw[i] else None for i in range(n)]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("lo", [0, 1, 1000])
def test_against_the_parents_table(eg, T, grp, small, multiples, bits, lo):
    """Every m in [lo, lo + 5000), the elements just outside, negated ones and 64 random elements: found and values equal
    eg_dlog_table_get's on a table of the same range."""
    hi = lo + 5000
    rnd = random.Random(100 * bits + lo)
    outside = [multiples[m] for m in (lo - 2, lo - 1, hi, hi + 1, hi + 2) if m > 0]
    negated = [grp.mul_generator(sc(-m)) for m in (1, lo + 1, lo + 2500, hi - 1, hi)]
    randoms = [grp.mul_generator(sc(rnd.randrange(L))) for _ in range(64)]
    elements = multiples[lo:hi] + outside + negated + randoms
    table = T.DiscreteLogTable(grp, range(lo, hi))
    want = table_get(eg, table, elements)
    table.close()
    assert want[:5000] == list(range(lo, hi)) and want[5000 + len(outside):] == [None] * (len(negated) + 64)
    assert small[bits].solve(elements, lo, hi) == want


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("m", [2**32, 2**40 - 1, 2**63, 2**64 - 2])
def test_against_the_oracle_in_windows_around_large_values(oracle, small, bits, m):
    """Elements [v]G by the oracle's generator multiplication (no GPU involved), each solved in a window around m whose lo is no multiple
    of the step: the window's first and last value, both sides of the first three giant-step boundaries and of a run boundary, and m."""
    W = 1 << bits
    span = (RUN + 3) * W + 5
    lo = min(m - 777, TOP - span)
    hi = lo + span
    assert lo % W != 0 and lo <= m < hi <= TOP
    inside = [lo, hi - 1, m, lo + RUN * W - 1, lo + RUN * W]
    for k in (1, 2, 3):
        inside += [lo + k * W - 1, lo + k * W]
    outside = [lo - 1, hi] + ([hi + 1] if hi + 1 < 2**64 else [])
    elements = [oracle.point_mul_generator(sc(v)) for v in inside + outside]
    assert small[bits].solve(elements, lo, hi) == inside + [None] * len(outside)
    assert small[bits].solve(elements[2:3], m, m + 1) == [m] and small[bits].solve(elements[2:3], m, m) == [None]


def test_identity_is_zero_whatever_the_range(small, default_solver):
    for s in (small[8], default_solver):
        assert s.solve([ZERO], 5, 100) == [0] and s.solve([ZERO], 0, 100) == [0] and s.solve([ZERO], 7, 7) == [0]
        assert s.solve([ZERO], TOP - 1, TOP) == [0]


def test_rejected_encodings_are_not_found_and_disturb_nothing(small, multiples, rejections):
    """The reference's own rejecting inputs and non-canonical encodings: found = 0, the call returns EG_OK, neighbours are answered."""
    bad = sorted({bytes.fromhex(v["hex"]) for k, v in rejections.items() if not k.startswith("_")})
    bad.append(P.to_bytes(32, "little"))                                        # zero, written non-canonically
    bad.append((int.from_bytes(multiples[9], "little") | 1 << 255).to_bytes(32, "little"))      # a valid element with bit 255 set
    bad.append((int.from_bytes(multiples[9], "little") + 1).to_bytes(32, "little"))             # a negative field element
    assert small[8].solve(bad, 0, 3000) == [None] * len(bad)
    batch, want = [], []
    for i, b in enumerate(bad):
        batch += [multiples[100 + 300 * i], b, multiples[2999 - i]]
        want += [100 + 300 * i, None, 2999 - i]
    assert small[8].solve(batch, 0, 3000) == want
    assert small[10].solve(batch, 0, 3000) == want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4000, 2**17 + 5])
def test_answers_do_not_depend_on_position(small, multiples, n):
    """Batches with duplicates: each answer is that of its element alone (2^17 + 5: more elements than one launch has lanes, so the
    call is cut into two blocks of elements, and every element of a block is answered in one launch)."""
    lo, hi = 17, 4017
    pool = [(multiples[m], m if lo <= m < hi else None) for m in (17, 18, 272, 273, 1000, 2064, 4016, 4017, 16, 5000)] + [(ZERO, 0)]
    rnd = random.Random(n)
    picks = [pool[rnd.randrange(len(pool))] for _ in range(n)]
    assert small[8].solve([p[0] for p in picks], lo, hi) == [p[1] for p in picks]
    assert small[10].solve([p[0] for p in reversed(picks)], lo, hi) == [p[1] for p in reversed(picks)]


def test_default_solver_in_a_span_of_2_40(oracle, default_solver):
    lo = 123_456_789
    hi = lo + 2**40
    inside = [lo, lo + 1, hi - 1, hi - 2, lo + 2**39, lo + 2**39 + 1, lo + 2**24 - 1, lo + 2**24, lo + 3 * 2**30 + 7, lo + 2**40 - 2**24,
              lo + 987_654_321_098, lo + 5, lo + 2**33, lo + 2**36 + 2**12, lo + 2**38 - 1]
    values = inside[:7] + [hi + 5] + inside[7:]
    assert len(values) == 16
    elements = [oracle.point_mul_generator(sc(v)) for v in values]
    assert default_solver.max_span(16) >= 2**40 and default_solver.table_bytes > 0
    assert default_solver.solve(elements, lo, hi) == inside[:7] + [None] + inside[7:]


def test_refusals(eg, T, grp, small, multiples):
    s = small[8]
    with pytest.raises(eg.EgError):
        s.solve([multiples[5]], 10, 9)
    wide = s.max_span(3)
    assert s.solve([multiples[5]] * 3, 0, wide) == [5] * 3
    with pytest.raises(eg.EgError, match="baby_bits"):
        s.solve([multiples[5]] * 3, 0, wide + 1)
    with pytest.raises(eg.EgError, match="baby_bits"):
        s.solve([multiples[5]], 0, TOP)
    lib = eg._load()
    v, f = (C.c_uint64 * 1)(), C.create_string_buffer(1)
    assert lib.eg_dlog_solver_solve(s._h, 1, None, 0, 10, v, f) == -3
    assert lib.eg_dlog_solver_solve(s._h, 1, multiples[5], 0, 10, None, f) == -3
    assert lib.eg_dlog_solver_solve(s._h, 1, multiples[5], 0, 10, v, None) == -3
    assert lib.eg_dlog_solver_solve(None, 1, multiples[5], 0, 10, v, f) == -3
    assert lib.eg_dlog_solver_solve(s._h, 0, None, 0, 10, None, None) == 0          # nothing to answer
    assert lib.eg_dlog_solver_create(grp.ctx._h, 12, None) == -3
    for bits in (7, 29, -1):
        with pytest.raises(eg.EgError):
            T.DiscreteLogSolver(grp, bits)


def test_two_solvers_and_a_verify_call_from_three_threads(eg, ctx, oracle, small, multiples, golden):
    import base64

    pk = base64.urlsafe_b64decode(golden["public_key_b64"] + "=" * (-len(golden["public_key_b64"]) % 4))
    params = eg.ChoiceParams(ctx, pk, 5, True)
    ballots = params.encrypt_batch(77, 0, 64)
    lo, hi = 3, 5003
    elements = multiples[0:6000:7]
    want = [m if lo <= m < hi else (0 if m == 0 else None) for m in range(0, 6000, 7)]
    alone = (small[8].solve(elements, lo, hi), small[10].solve(elements, lo, hi), params.verify_batch(ballots)[0])
    assert alone[0] == want and alone[1] == want and alone[2] == [0] * 64
    got, errors = {}, []

    def run(name, fn):
        try:
            for _ in range(3):
                got.setdefault(name, []).append(fn())
        except Exception as e:          # noqa: BLE001 - reported below
            errors.append((name, e))

    threads = [threading.Thread(target=run, args=("s8", lambda: small[8].solve(elements, lo, hi))),
               threading.Thread(target=run, args=("s10", lambda: small[10].solve(elements, lo, hi))),
               threading.Thread(target=run, args=("verify", lambda: params.verify_batch(ballots)[0]))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got["s8"] == [alone[0]] * 3 and got["s10"] == [alone[1]] * 3 and got["verify"] == [alone[2]] * 3


def test_threshold_tally_read_through_the_solver(eg, T, ctx, grp, oracle, default_solver):
    """The 7-of-10 threshold tally of test_threshold_tally_end_to_end's shape: the totals read through decrypt_totals over [0, 2^40) - a
    range no table holds - equal the totals read through the table."""
    rnd = random.Random(2025)
    shares_n, threshold, n_opt, votes = 10, 7, 5, 60
    coeffs = [rnd.randrange(L) for _ in range(threshold)]
    f = lambda x: sum(c * pow(x, k, L) for k, c in enumerate(coeffs)) % L
    sk_shares = [f(i + 1) for i in range(shares_n)]
    shared_key = oracle.point_mul_generator(sc(coeffs[0]))
    params = eg.ChoiceParams(ctx, shared_key, n_opt, True)
    ballots = params.encrypt_batch(91, 0, votes)
    expected = [0] * n_opt
    for i in range(votes):
        expected[oracle.select_single(91 + i, n_opt).index(1)] += 1
    st, totals = params.verify_batch(ballots)
    assert st == [0] * votes
    cts = [totals[64 * k : 64 * k + 64] for k in range(n_opt)]
    dhs = []
    for ct in cts:
        shares = [(i, oracle.point_multi_mul(sc(sk_shares[i]), ct[:32])) for i in rnd.sample(range(shares_n), threshold)]
        dhs.append(T.combine_shares(grp, threshold, shares, n_shares=shares_n))
    table = T.DiscreteLogTable(grp, range(votes + 1))
    through_table = [T.decrypt_total(grp, table, ct, dh) for ct, dh in zip(cts, dhs)]
    table.close()
    assert through_table == expected and sum(expected) == votes
    assert T.decrypt_totals(grp, default_solver, cts, dhs, 0, 2**40) == through_table
    assert T.decrypt_totals(grp, default_solver, cts, dhs, max(expected) + 1, 2**40) == [None if v else 0 for v in expected]


def test_solving_is_faster_than_building_the_parents_table(eg, T, grp, oracle, default_solver):
    """The point of the feature: 16 elements in a span of 2^24 with a ready solver against eg_dlog_table_create over 2^20 values - the
    parent's path on a sixteenth of the range.  Medians of 5 runs after a warm-up, same process."""
    lo, hi = 1, 1 + 2**24
    values = [lo + (k * (2**24 - 1)) // 15 for k in range(16)]
    elements = [oracle.point_mul_generator(sc(v)) for v in values]
    lib = eg._load()
    table_values = (C.c_uint64 * 2**20)(*range(1, 2**20 + 1))

    def solve():
        t = time.perf_counter()
        assert default_solver.solve(elements, lo, hi) == values
        return time.perf_counter() - t

    def create():
        h = C.c_void_p()
        t = time.perf_counter()
        eg._check(lib.eg_dlog_table_create(grp.ctx._h, 2**20, table_values, C.byref(h)))
        dt = time.perf_counter() - t
        lib.eg_dlog_table_destroy(h)
        return dt

    solve(), create()
    t_solve = sorted(solve() for _ in range(5))[2]
    t_create = sorted(create() for _ in range(5))[2]
    print(f"solve 16 elements in a span of 2^24: {t_solve * 1e3:.3f} ms; eg_dlog_table_create over 2^20 values: {t_create * 1e3:.1f} ms")
    assert t_solve < t_create
