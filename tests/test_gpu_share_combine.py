"""The batched share combination (eg_combine_shares_batch[_device], tally.combine_shares_batch / decrypt_tallies) on the GPU.  Key sets,
ciphertexts and every expected value come from the CPU oracle or from its restatement of the reference (tests/share_combine_ref.py):
dh = [x]R by oracle.point_multi_mul, plain = [count]G by oracle.point_mul_generator, selection and counters by R.expected - never from
the library under test, except where the issue asks for byte equality with eg_combine_shares + element_add on the same shares."""
import random
import threading
import time

import numpy as np
import pytest

import share_combine_ref as R

pytestmark = pytest.mark.gpu

sc = R.sc
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def eg():
    import elastic_elgamal_amd as m

    return m


@pytest.fixture(scope="module")
def T():
    from elastic_elgamal_amd import tally

    return tally


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
def grp(eg, ctx):
    return eg.Ristretto(ctx)


def dev(torch, data: bytes):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def u32(torch, values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def run_device(torch, T, grp, shares_n, threshold, cts, indexes, columns, status, stream=0, with_dh=True, with_plain=True, with_used=True):
    """the device entry with buffers of its own -> (dh, plain, combined, used, bad) as the restatement gives them (an output that was
    not asked for comes back as None after its sentinel was found untouched); a 4 KiB canary behind the scratch must survive"""
    m, k = len(cts), len(indexes)
    d_cts = dev(torch, b"".join(cts)) if m else None
    d_items = dev(torch, b"".join(b"".join(col) for col in columns)) if m and k else None
    d_status = u32(torch, [s for col in status for s in col]) if status is not None and m and k else None
    need = T.combine_shares_batch_scratch_bytes(threshold, m)
    scratch = torch.full((need + 4096,), 0x5C, dtype=torch.uint8, device="cuda")
    dh = torch.full((max(m, 1), 32), 0xAB, dtype=torch.uint8, device="cuda")
    plain = torch.full((max(m, 1), 32), 0xAB, dtype=torch.uint8, device="cuda")
    combined = torch.full((max(m, 1),), 0x77, dtype=torch.uint8, device="cuda")
    used = torch.full((max(m, 1),), -1, dtype=torch.int64, device="cuda")
    bad = torch.full((4,), 77, dtype=torch.int32, device="cuda")              # the library WRITES the first three words
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() if t is not None else 0
    T.combine_shares_batch_device(grp, shares_n, threshold, m, ptr(d_cts), indexes, ptr(d_items), ptr(d_status), combined.data_ptr(),
                                  bad.data_ptr(), scratch.data_ptr(), d_dh=dh.data_ptr() if with_dh else 0,
                                  d_plain=plain.data_ptr() if with_plain else 0, d_used=used.data_ptr() if with_used else 0, stream=stream)
    torch.cuda.synchronize()
    assert bool((scratch[need:] == 0x5C).all().item()), "the pass wrote behind its scratch"
    assert bad.cpu().tolist()[3] == 77
    rows = lambda t: [bytes(r) for r in t.cpu().numpy()[:m]]
    if not with_dh:
        assert bool((dh == 0xAB).all().item())
    if not with_plain:
        assert bool((plain == 0xAB).all().item())
    if not with_used:
        assert bool((used == -1).all().item())
    return (rows(dh) if with_dh else None, rows(plain) if with_plain else None, combined.cpu().tolist()[:m],
            [x & M64 for x in used.cpu().tolist()[:m]] if with_used else None, tuple(bad.cpu().tolist()[:3]))


class Corpus:
    """m ciphertexts of known counts under a key set, every participant's items made by eg_share_prove_batch and checked by
    eg_verify_proof_batch (the flow of a tally stage), and what the oracle says they open to"""

    def __init__(self, eg, ctx, oracle, shares_n, threshold, m, seed):
        self.shares, self.threshold, self.m = shares_n, threshold, m
        self.ks = R.KeySet(oracle, shares_n, threshold, seed)
        self.counts = [0, 1, 2] + [(7919 * c + seed) % 100000 for c in range(3, m)]
        self.counts = self.counts[:m]
        self.cts = R.ciphertexts(oracle, self.ks, self.counts, seed + 1)
        self.Rs = b"".join(ct[:32] for ct in self.cts)
        self.verifiers = [eg.DecryptionShareVerifier(ctx, self.ks.shared_key, shares_n, threshold, i, self.ks.part_keys[i]) for i in range(shares_n)]
        self.columns, self.status = [], []
        for i, ver in enumerate(self.verifiers):
            items, ok = ver.prove(sc(self.ks.sks[i]), seed + 100 * i, 0, self.Rs)
            assert set(ok) == {1}
            self.columns.append([items[128 * c:128 * c + 128] for c in range(m)])
            self.status.append(ver.verify_batch(items))
        assert all(s == [0] * m for s in self.status)
        self.x_R = [oracle.point_multi_mul(sc(self.ks.secret), ct[:32]) for ct in self.cts]
        self.plains = [oracle.point_mul_generator(sc(v)) for v in self.counts]

    def mask(self, participants):
        return sum(1 << i for i in participants)


@pytest.fixture(scope="module")
def base(eg, ctx, oracle):
    """7-of-10, 257 ciphertexts: the sizes of the tests are prefixes of it"""
    b = Corpus(eg, ctx, oracle, 10, 7, 257, 7010)
    assert b.plains[0] == bytes(32) and b.counts[0] == 0
    assert oracle.decryption_share_verify(b.ks.part_keys[3], 10, 7, b.ks.shared_key, 3, b.columns[3][5]) == 0      # the oracle accepts them too
    return b


def prefix(b, m, cols=None):
    cols = list(range(b.shares)) if cols is None else cols
    return b.cts[:m], cols, [b.columns[j][:m] for j in cols], [b.status[j][:m] for j in cols]


# ------------------------------------------------------------------ 1. sizes and key sets
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_sizes_at_7_of_10(torch, T, grp, oracle, base, m):
    """one lane, both sides of a wavefront, more than one block: dh = [x]R, plain = [count]G (32 zero bytes for the count 0, with
    combined = 1), the first seven of ten columns used"""
    cts, idx, cols, st = prefix(base, m)
    got = run_device(torch, T, grp, 10, 7, cts, idx, cols, st)
    assert got == R.expected(oracle, 10, 7, cts, idx, cols, st)
    assert got[0] == base.x_R[:m] and got[1] == base.plains[:m] and got[1][0] == bytes(32)
    assert got[2] == [1] * m and got[3] == [base.mask(range(7))] * m and got[4] == (0, 0, 0)


@pytest.mark.parametrize("shares_n,threshold", [(1, 1), (3, 2), (8, 8), (12, 9), (20, 17), (64, 64)])
def test_key_sets_at_65_ciphertexts(torch, T, grp, oracle, shares_n, threshold):
    """the smallest key set, both sides of the chunk seam (8 | 9, 16 | 17) and the largest: columns in shuffled order, proof-less items
    from the oracle and no status words (the pass reads R and dh of an item, nothing else)"""
    m = 65
    ks = R.KeySet(oracle, shares_n, threshold, 500 + shares_n)
    counts = [0, 1 << 40] + [3 * c for c in range(2, m)]
    cts = R.ciphertexts(oracle, ks, counts, shares_n)
    indexes = random.Random(shares_n).sample(range(shares_n), shares_n)
    needed = indexes[:threshold]                       # shares behind the threshold-th column are never looked at: leave them empty
    columns = [[ks.plain_item(oracle, i, ct[:32]) if i in needed else ct[:32] + bytes(96) for ct in cts] for i in indexes]
    got = run_device(torch, T, grp, shares_n, threshold, cts, indexes, columns, None)
    assert got[0] == [oracle.point_multi_mul(sc(ks.secret), ct[:32]) for ct in cts]
    assert got[1] == [oracle.point_mul_generator(sc(v)) for v in counts]
    assert got[2] == [1] * m and got[3] == [sum(1 << i for i in needed)] * m and got[4] == (0, 0, 0)


# ------------------------------------------------------------------ 2. agreement with the existing entry
def test_byte_equal_to_combine_shares_and_element_add(torch, T, grp, base):
    """eg_combine_shares + element_add on the same shares, ciphertext by ciphertext, give the batch entry's bytes"""
    m = 65
    cts, idx, cols, st = prefix(base, m, [9, 2, 5, 0, 7, 1, 3, 8])
    dh, plain, combined, used, bad = run_device(torch, T, grp, 10, 7, cts, idx, cols, st)
    assert combined == [1] * m and bad == (0, 0, 0)
    for c in range(m):
        one = T.combine_shares(grp, 7, [(i, cols[j][c][32:64]) for j, i in enumerate(idx)], n_shares=10)
        diff, ok = grp.element_add(cts[c][32:], one, subtract=True)
        assert (one, diff) == (dh[c], plain[c]) and set(ok) == {1}, c


# ------------------------------------------------------------------ 3. column order
def test_columns_in_shuffled_order_and_more_columns_than_needed(torch, T, grp, oracle, base):
    m = 65
    order = random.Random(5).sample(range(10), 10)
    for cols in (order, order[::-1], order[:7], list(range(10))):
        cts, idx, columns, st = prefix(base, m, cols)
        got = run_device(torch, T, grp, 10, 7, cts, idx, columns, st)
        assert got[0] == base.x_R[:m] and got[1] == base.plains[:m] and got[2] == [1] * m
        assert got[3] == [base.mask(cols[:7])] * m and got[4] == (0, 0, 0)       # all ten given, seven used: the first seven columns


# ------------------------------------------------------------------ 4. share selection
def test_one_rejected_share_in_the_middle_of_a_wavefront(torch, T, grp, oracle, base):
    """ciphertext 37 of 128 has a rejected share in column 2: its lane takes column 7 instead, its coefficients differ from all its
    neighbours', and its result is still [x]R"""
    m = 128
    cts, idx, cols, st = prefix(base, m)
    st = [list(s) for s in st]
    st[2][37] = 0x20001
    got = run_device(torch, T, grp, 10, 7, cts, idx, cols, st)
    assert got == R.expected(oracle, 10, 7, cts, idx, cols, st)
    assert got[0] == base.x_R[:m] and got[1] == base.plains[:m] and got[2] == [1] * m and got[4] == (0, 0, 0)
    assert got[3] == [base.mask(range(7))] * 37 + [base.mask([0, 1, 3, 4, 5, 6, 7])] + [base.mask(range(7))] * 90


def test_a_tenth_of_all_shares_tampered(torch, T, grp, oracle, base):
    """a tenth of the 10 x 257 items tampered in one bit and four more columns of three ciphertexts, status words from
    eg_verify_proof_batch itself: exactly the tampered items are rejected, every ciphertext with seven good shares opens to [x]R over
    exactly its first seven good columns, the others are not combined"""
    m, rnd = 257, random.Random(10)
    tampered = set(rnd.sample(range(10 * m), m))
    for c in (0, 100, 256):
        tampered |= {j * m + c for j in rnd.sample(range(10), 4)}
    columns, status = [], []
    for j, ver in enumerate(base.verifiers):
        col = [bytearray(x) for x in base.columns[j]]
        for c in range(m):
            if j * m + c in tampered:
                col[c][rnd.randrange(128)] ^= 1 << rnd.randrange(8)
        col = [bytes(x) for x in col]
        columns.append(col)
        status.append(ver.verify_batch(b"".join(col)))
    assert {j * m + c for j in range(10) for c in range(m) if status[j][c] != 0} == tampered
    got = run_device(torch, T, grp, 10, 7, base.cts, list(range(10)), columns, status)
    good = [[j for j in range(10) if j * m + c not in tampered] for c in range(m)]
    assert got[2] == [int(len(g) >= 7) for g in good] and 3 <= got[2].count(0) < m // 4
    assert got[3] == [base.mask(g[:7]) if len(g) >= 7 else 0 for g in good] and len(set(got[3])) > 10
    assert got[0] == [x if len(g) >= 7 else bytes(32) for x, g in zip(base.x_R, good)]
    assert got[1] == [p if len(g) >= 7 else bytes(32) for p, g in zip(base.plains, good)]
    assert got[4] == (0, 0, 0)
    assert got == R.expected(oracle, 10, 7, base.cts, list(range(10)), columns, status)


# ------------------------------------------------------------------ 5. hostile inputs
def test_hostile_inputs_at_the_lane_corners(torch, T, grp, oracle, base, rejections):
    """shares marked accepted that no verifier accepted, at lanes 0 / 63 / 64 / last: another ciphertext's share (bad[0], skipped, still
    [x]R), a decodable but wrong dh (the restatement over exactly the first seven usable columns, not [x]R), a dh and a B the reference
    rejects (bad[1], bad[2]: combined 0, zero bytes); the host form writes the same outputs and then fails"""
    non_element = bytes.fromhex(rejections["non_element"]["hex"])
    m = 130
    cts, idx, cols, st = prefix(base, m)
    cts, cols = list(cts), [list(c) for c in cols]
    cols[1][0] = cols[1][5]                                                      # lane 0: a true share of ciphertext 5
    cols[3][63] = cols[3][63][:32] + cols[3][62][32:64] + cols[3][63][64:]       # lane 63: the dh of its neighbour
    cols[6][64] = cols[6][64][:32] + non_element + cols[6][64][64:]              # lane 64: dh does not decode
    cts[m - 1] = cts[m - 1][:32] + non_element                                   # last lane: B does not decode
    cols[9][7] = cols[9][7][:32] + non_element + bytes(64)                       # behind the seventh usable column: never decoded
    got = run_device(torch, T, grp, 10, 7, cts, idx, cols, st)
    want = R.expected(oracle, 10, 7, cts, idx, cols, st)
    assert got == want and got[4] == (1, 1, 1)
    assert got[0][0] == base.x_R[0] and got[3][0] == base.mask([0, 2, 3, 4, 5, 6, 7])
    assert got[0][63] == R.combine_shares(oracle, 10, 7, [(j, cols[j][63][32:64]) for j in range(7)]) != base.x_R[63]
    assert got[2] == [1] * 64 + [0] + [1] * 64 + [0] and got[0][64] == got[1][64] == got[0][m - 1] == got[1][m - 1] == bytes(32)
    assert got[3][64] == got[3][m - 1] == 0
    # without d_plain, B is not decoded
    dh_only = run_device(torch, T, grp, 10, 7, cts, idx, cols, st, with_plain=False)
    assert dh_only[4] == (1, 1, 0) and dh_only[2][m - 1] == 1 and dh_only[0][m - 1] == base.x_R[m - 1]


def test_host_form_reports_hostile_inputs(eg, T, grp, base, rejections):
    m = 3
    cts, idx, cols, st = prefix(base, m)
    cols = [list(c) for c in cols]
    cols[0][1] = cols[0][1][:32] + bytes.fromhex(rejections["non_element"]["hex"]) + cols[0][1][64:]
    with pytest.raises(eg.EgError, match="1 chosen share"):
        T.combine_shares_batch(grp, 10, 7, b"".join(cts), idx, b"".join(b"".join(c) for c in cols), [s for col in st for s in col])


# ------------------------------------------------------------------ 6. argument variants and entry forms
def test_argument_variants(torch, T, grp, oracle, base):
    m = 65
    cts, idx, cols, st = prefix(base, m)
    full = run_device(torch, T, grp, 10, 7, cts, idx, cols, st)
    assert run_device(torch, T, grp, 10, 7, cts, idx, cols, None) == full                         # d_status == NULL
    for off in ("with_dh", "with_plain", "with_used"):                                           # each output NULL: the others unchanged
        got = run_device(torch, T, grp, 10, 7, cts, idx, cols, st, **{off: False})
        position = {"with_dh": 0, "with_plain": 1, "with_used": 3}[off]
        assert got[position] is None and [g for i, g in enumerate(got) if i != position] == [f for i, f in enumerate(full) if i != position]
    for k in (6, 1, 0):                                                                          # k < threshold: valid, nothing combined
        got = run_device(torch, T, grp, 10, 7, cts, idx[:k], cols[:k], st[:k])
        assert got == ([bytes(32)] * m, [bytes(32)] * m, [0] * m, [0] * m, (0, 0, 0))
    assert run_device(torch, T, grp, 10, 7, [], idx, [[] for _ in idx], None) == ([], [], [], [], (0, 0, 0))      # m == 0
    assert T.combine_shares_batch(grp, 10, 7, b"", idx, b"") == (b"", b"", [], [])


def test_both_entry_forms_and_a_caller_stream_twice(torch, T, grp, base):
    m = 65
    cts, idx, cols, st = prefix(base, m, [4, 8, 1, 9, 0, 6, 2, 3])
    flat = [s for col in st for s in col]
    dh, plain, combined, used = T.combine_shares_batch(grp, 10, 7, b"".join(cts), idx, b"".join(b"".join(c) for c in cols), flat)
    assert dh == b"".join(base.x_R[:m]) and plain == b"".join(base.plains[:m]) and combined == [1] * m and used == [base.mask(idx[:7])] * m
    s = torch.cuda.Stream()
    for stream in (s.cuda_stream, s.cuda_stream, 0):
        got = run_device(torch, T, grp, 10, 7, cts, idx, cols, st, stream=stream)
        assert (b"".join(got[0]), b"".join(got[1]), got[2], got[3], got[4]) == (dh, plain, combined, used, (0, 0, 0))


def test_refusals_with_a_context(torch, eg, T, grp):
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    good = dict(shares=3, threshold=2, m=4, d_ciphertexts=p, indexes=[0, 2], d_items=p, d_status=p, d_combined=p, d_bad=p, d_scratch=p)
    for change, message in ((dict(shares=0), "EG_COMBINE_SHARES_MAX"), (dict(shares=65), "EG_COMBINE_SHARES_MAX"), (dict(threshold=4), "threshold"),
                            (dict(threshold=0), "threshold"), (dict(indexes=[0, 1, 2, 0]), "k is outside"), (dict(indexes=[0, 3]), "index exceeds"),
                            (dict(indexes=[2, 2]), "duplicate"), (dict(m=1 << 31), "2\\^31"), (dict(d_ciphertexts=0), "null"), (dict(d_items=0), "null"),
                            (dict(d_combined=0), "null"), (dict(d_bad=0), "null"), (dict(d_scratch=0), "null scratch"),
                            (dict(d_items=p + 8), "16-byte aligned"), (dict(d_scratch=p + 4), "16-byte aligned"), (dict(d_used=p + 4), "8-byte aligned")):
        with pytest.raises(eg.EgError, match=message):
            T.combine_shares_batch_device(grp, **{**good, **change})
    torch.cuda.synchronize()
    assert not bool(buf.any().item())                  # refused before anything was launched


# ------------------------------------------------------------------ 7. concurrency
def test_a_pass_beside_a_verifying_thread_on_the_same_context(torch, T, grp, base):
    m = 257
    cts, idx, cols, st = prefix(base, m)
    items0 = b"".join(base.columns[0])
    errors, out = [], {}

    def verifier():
        try:
            out["status"] = [base.verifiers[0].verify_batch(items0) for _ in range(4)]
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    def combiner():
        try:
            s = torch.cuda.Stream()
            out["runs"] = [run_device(torch, T, grp, 10, 7, cts, idx, cols, st, stream=s.cuda_stream) for _ in range(3)]
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=verifier), threading.Thread(target=combiner)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert out["status"] == [[0] * m] * 4
    for got in out["runs"]:
        assert got[0] == base.x_R and got[1] == base.plains and got[2] == [1] * m and got[4] == (0, 0, 0)


# ------------------------------------------------------------------ 8. end to end
def test_decrypt_tallies_over_the_grouped_tally_of_a_verified_batch(eg, ctx, T, grp, oracle):
    """350 ballots in 7 precincts under a 7-of-10 key: batch verify, grouped tally, every participant's shares of the 35 ciphertexts by
    eg_share_prove_batch, decrypt_tallies -> the per-precinct counts, which add up to the overall result"""
    votes, n_opt, n_groups = 350, 5, 7
    ks = R.KeySet(oracle, 10, 7, 31)
    params = eg.ChoiceParams(ctx, ks.shared_key, n_opt, True)
    ballots = bytearray(params.encrypt_batch(77, 0, votes))
    ballots[13 * params.ballot_size + 40] ^= 4                  # one ballot no verifier accepts
    ballots = bytes(ballots)
    status, overall = params.verify_batch(ballots)
    assert [b for b, s in enumerate(status) if s] == [13]
    groups = [(b * 5 + b // 9) % n_groups for b in range(votes)]
    expected = [[0] * n_opt for _ in range(n_groups)]
    for b in range(votes):
        if b != 13:
            expected[groups[b]][oracle.select_single(77 + b, n_opt).index(1)] += 1
    tallies, counts = params.tally_grouped(ballots, status, groups, n_groups)
    assert sum(counts) == votes - 1
    Rs = b"".join(tallies[64 * c:64 * c + 32] for c in range(n_groups * n_opt))
    verifiers = [(i, eg.DecryptionShareVerifier(ctx, ks.shared_key, 10, 7, i, ks.part_keys[i])) for i in (8, 3, 0, 9, 5, 1, 6, 2)]
    items = [ver.prove(sc(ks.sks[i]), 900 + i, 0, Rs)[0] for i, ver in verifiers]
    spoiled = bytearray(items[1])
    spoiled[128 * 4 + 70] ^= 1                                  # participant 3's share of ciphertext 4 does not verify
    items[1] = bytes(spoiled)
    solver = T.DiscreteLogSolver(grp, 12)
    values, combined, used, st = T.decrypt_tallies(grp, 10, 7, tallies, verifiers, items, solver=solver, lo=0, hi=votes + 1)
    assert [values[n_opt * g:n_opt * g + n_opt] for g in range(n_groups)] == expected and combined == [1] * (n_groups * n_opt)
    first7 = sum(1 << i for i, _ in verifiers[:7])
    assert used == [first7] * 4 + [first7 - (1 << 3) + (1 << 2)] + [first7] * 30 and sum(1 for s in st if s) == 1
    table = T.DiscreteLogTable(grp, range(votes + 1))
    assert T.decrypt_tallies(grp, 10, 7, tallies, verifiers, items, table=table)[0] == values
    # ... and the precincts add up to the overall result, opened the same way
    o_items = [ver.prove(sc(ks.sks[i]), 950 + i, 0, b"".join(overall[64 * t:64 * t + 32] for t in range(n_opt)))[0] for i, ver in verifiers]
    totals = T.decrypt_tallies(grp, 10, 7, overall, verifiers, o_items, solver=solver, lo=0, hi=votes + 1)[0]
    assert totals == [sum(expected[g][t] for g in range(n_groups)) for t in range(n_opt)] and sum(totals) == votes - 1
    # too few verifiers: nothing opens
    assert T.decrypt_tallies(grp, 10, 7, tallies, verifiers[:6], items[:6], table=table)[0] == [None] * (n_groups * n_opt)
    solver.close()
    table.close()


# ------------------------------------------------------------------ 9. timing
def test_batch_entry_beats_the_calls_it_replaces(torch, T, grp, base):
    """m = 256 at 7-of-10: the batch entry on device buffers (call + synchronise) against the 256 eg_combine_shares calls it
    replaces, both warmed up, in the same process.  The only condition is a ratio above 1 (tools/share_combine_probe.py records it)."""
    m = 256
    cts, idx, cols, st = prefix(base, m, list(range(7)))
    d_cts = dev(torch, b"".join(cts))
    d_items = dev(torch, b"".join(b"".join(c) for c in cols))
    d_status = u32(torch, [s for col in st for s in col])
    scratch = torch.empty(T.combine_shares_batch_scratch_bytes(7, m), dtype=torch.uint8, device="cuda")
    dh = torch.zeros((m, 32), dtype=torch.uint8, device="cuda")
    plain = torch.zeros((m, 32), dtype=torch.uint8, device="cuda")
    combined = torch.zeros(m, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(4, dtype=torch.int32, device="cuda")

    def batch():
        T.combine_shares_batch_device(grp, 10, 7, m, d_cts.data_ptr(), idx, d_items.data_ptr(), d_status.data_ptr(), combined.data_ptr(),
                                      bad.data_ptr(), scratch.data_ptr(), d_dh=dh.data_ptr(), d_plain=plain.data_ptr())
        torch.cuda.synchronize()

    shares = [[(i, cols[j][c][32:64]) for j, i in enumerate(idx)] for c in range(m)]

    def one_by_one():
        return [T.combine_shares(grp, 7, shares[c], n_shares=10) for c in range(m)]

    batch()
    one_by_one()[:8]
    t0 = time.perf_counter()
    batch()
    t1 = time.perf_counter()
    singles = one_by_one()
    t2 = time.perf_counter()
    assert [bytes(r) for r in dh.cpu().numpy()] == singles == base.x_R[:m] and combined.cpu().tolist() == [1] * m
    ratio = (t2 - t1) / (t1 - t0)
    print(f"share combine, m = 256, 7-of-10: batch entry {1e3 * (t1 - t0):.3f} ms, 256 eg_combine_shares calls {1e3 * (t2 - t1):.1f} ms, ratio {ratio:.1f}")
    assert ratio > 1
