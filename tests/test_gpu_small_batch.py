"""The small-batch entries (eg_verify_*_small[_device]: one workgroup per ballot in one launch, four lanes per point operation) on the
GPU: the quad operations limb for limb against the bound-check host build, verdicts and tallies against the oracle and against
eg_verify_*_batch on the same bytes for every election shape, the reference's snapshots, the edge corpus, tally semantics, entry forms,
concurrency with the batch path, and the latency relation that is the point of the path: faster than the batch entry on the same chip.

Packed ballots have a fixed shape, so the length-mismatch variants (Range(LenMismatch), Variant(LenMismatch), ...) cannot occur on
this path: the batch entries never produce them either (they belong to the object ingest)."""
import ctypes as C
import random
import statistics
import subprocess
import threading
import time
from pathlib import Path

import pytest

import edge_ballots as E
import limb_cases as lc

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
SIZES = (1, 2, 3, 4, 63, 64, 65, 255, 256, 1000, 4096)


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
def pk(golden):
    import base64

    s = golden["public_key_b64"]
    return base64.urlsafe_b64decode(s + "=" * (-len(s) % 4))


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


# ------------------------------------------------------------------ quad operations: device == host build, limb for limb
def test_quad_operations_device_equals_host_build_limb_for_limb():
    """every quad operation on the limb-corner inputs of tests/limb_cases.py: the device build (tests/quaddev, four adjacent lanes per
    case, DPP exchanges) returns exactly the limbs of the bound-check host build (a quad emulated as four lanes), which asserts the
    preconditions on the way"""
    import test_quad_arith_cpu as Q

    subprocess.check_call(["make", "-C", str(HERE / "quaddev")], stdout=subprocess.DEVNULL)
    srcs = [Q.SRC, HERE / "quaddev" / "quad_ops.cuh"] + list((HERE.parent / "elastic_elgamal_amd" / "csrc").glob("*.cuh"))
    if not Q.LIB.exists() or any(s.stat().st_mtime > Q.LIB.stat().st_mtime for s in srcs):
        subprocess.check_call(Q.CMD + ["-o", str(Q.LIB), str(Q.SRC)])
    host = C.CDLL(str(Q.LIB))
    dev = C.CDLL(str(HERE / "quaddev" / "libquaddev.so"))
    assert dev.qd_quad_op_count() == len(Q.OP)
    for op, code in Q.OP.items():
        rng = random.Random(code + 100)
        ca, cb = Q.CLASSES[op]
        classes = list(ca) + list(cb or ())
        cases, want = [], []
        for name, operands in lc.family(classes, rng, 1100, additive_slack=False):
            if name == "hair" and any(c != 1 for c in classes):
                operands = [o if c == 1 else [min(v, lc.top(c, i)) for i, v in enumerate(o)] for o, c in zip(operands, classes)]
            if name == "slack" and op in ("cached_cneg", "neg", "to_cached", "add", "madd", "cached_neg_t"):
                continue
            a, b = operands[:4], (operands[4:] if cb else [[0] * lc.NL] * 4)
            got_q, _ = Q.run_op(host, op, a, [float(c) for c in ca], b, [float(c) for c in cb] if cb else None)
            if op == "cached_to_p2":
                got_q[3] = None            # T is not produced: whatever lane 3 holds is not part of the result
            cases.append([v for fe in a + b for v in fe])
            want.append(got_q)
        n = len(cases)
        assert n >= 1000 and n % 64 != 0
        flat = (C.c_uint32 * (72 * n))(*[v for c in cases for v in c])
        for block in (64, 256):
            out = (C.c_uint32 * (36 * n))()
            assert dev.qd_quad_ops(code, n, flat, out, block) == 0, (op, block)
            for i in range(n):
                for r in range(4):
                    if want[i][r] is not None:
                        assert list(out[36 * i + 9 * r : 36 * i + 9 * r + 9]) == want[i][r], (op, block, i, r)


# ------------------------------------------------------------------ parity: every shape, every size, tampering
class Shape:
    def __init__(self, eg, ctx, oracle, pk, kind, n_options, arg):
        self.kind, self.n_options = kind, n_options
        if kind == "qv":
            self.op = oracle.QvParams(pk, n_options, arg)
            self.p = eg.QuadraticVotingParams(ctx, pk, n_options, arg)
        else:
            self.op = oracle.ChoiceParams(pk, n_options, kind == "single")
            self.p = eg.ChoiceParams(ctx, pk, n_options, kind == "single")
            self.n_selected = arg
        self.size = self.p.ballot_size
        assert self.size == self.op.ballot_size

    def generate(self, torch, seed, n):
        """n ballots from the GPU prover (bit-exact with the oracle's, tests/test_gpu_parity.py)"""
        out = torch.zeros(n * self.size, dtype=torch.uint8, device="cuda")
        if self.kind == "qv":
            self.p.encrypt_batch_device(seed, 0, n, out.data_ptr())
        else:
            self.p.encrypt_batch_device(seed, 0, n, out.data_ptr(), n_selected=self.n_selected)
        self.p.ctx.synchronize()
        return bytes(out.cpu().numpy())

    def classify_items(self, oracle, ballot):
        """which 32-byte items are points / scalars: the oracle's verdict on an item of 0xff bytes"""
        if hasattr(self, "_items"):
            return self._items
        pts, scs = [], []
        for it in range(self.size // 32):
            b = bytearray(ballot)
            b[32 * it : 32 * it + 32] = b"\xff" * 32
            st = self.op.verify(bytes(b))
            assert (st & 0xFF) in (1, 2) and st >> 8 == it, (it, hex(st))
            (pts if (st & 0xFF) == 2 else scs).append(it)
        self._items = (pts, scs)
        return pts, scs

    def tamperings(self, oracle, ballot):
        """[(name, function(bytearray ballot))]: every status variant a packed ballot can get"""
        pts, scs = self.classify_items(oracle, ballot)
        g = oracle.const_bytes(4)

        def bad_point(it):
            def f(b):
                b[32 * it : 32 * it + 32] = b"\xff" * 32
            return f

        def bad_scalar(it):
            def f(b):
                b[32 * it + 31] = 0xFF
            return f

        def add_g(off):
            def f(b):
                b[off : off + 32] = oracle.point_add(bytes(b[off : off + 32]), g)
            return f

        def flip(off, bit=1):
            def f(b):
                b[off] ^= bit
            return f

        out = [(f"bad_point_{w}", bad_point(it)) for w, it in (("first", pts[0]), ("middle", pts[len(pts) // 2]), ("last", pts[-1]))]
        out += [(f"bad_scalar_{w}", bad_scalar(it)) for w, it in (("first", scs[0]), ("middle", scs[len(scs) // 2]), ("last", scs[-1]))]
        if self.kind == "qv":
            vs = self.op.vote_size
            out += [(f"variant_{k}", add_g(k * vs + 32)) for k in range(self.n_options)]
            out.append(("credit_range", add_g(self.n_options * vs + 32)))
            out.append(("credit_equivalence", flip(self.size - 32)))
        else:
            n = self.n_options
            out.append(("range_challenge", flip(64 * n, 0x10)))                      # the common challenge
            out.append(("range_response", flip(64 * n + 32 * (1 + n), 1)))
            out.append(("range_ciphertext", add_g(32)))
            if self.kind == "single":
                out.append(("sum_challenge", flip(self.size - 32, 4)))               # the sum proof's response
        return out

    def close(self):
        self.p.close()


SHAPES = [("single", 2, 0), ("single", 3, 0), ("single", 5, 0), ("single", 10, 0), ("single", 15, 0), ("single", 150, 0), ("multi", 16, 3),
          ("qv", 5, 20), ("qv", 2, 4), ("qv", 4, 100)]            # the last two: from test_qv_unusual_parameters' list


@pytest.mark.parametrize("kind,n_options,arg", SHAPES)
def test_small_entries_equal_batch_entries_and_oracle(eg, ctx, oracle, pk, torch, kind, n_options, arg):
    """statuses AND tally bytes of the small entry == the batch entry on the same bytes (every ballot) == the oracle (every tampered
    ballot, every ballot of the batches up to 256, a random sample of the rest); a tenth of every batch is tampered, at positions 0,
    n - 1 and random ones, and over the sizes every status variant of the shape occurs"""
    sh = Shape(eg, ctx, oracle, pk, kind, n_options, arg)
    try:
        rnd = random.Random(f"{kind}{n_options}")
        pool = sh.generate(torch, 31337 + n_options, max(SIZES))
        tampers = sh.tamperings(oracle, pool[: sh.size])
        seen, next_tamper = set(), 0
        for n in SIZES:
            b = bytearray(pool[: n * sh.size])
            bad = {0, n - 1} | {rnd.randrange(n) for _ in range(max(0, n // 10 - 2))}      # n = 2: both ballots; n = 3, 4: the ends
            for i in sorted(bad):
                one = bytearray(b[i * sh.size : (i + 1) * sh.size])
                tampers[next_tamper % len(tampers)][1](one)
                next_tamper += 1
                b[i * sh.size : (i + 1) * sh.size] = one
            b = bytes(b)
            got, tally = sh.p.verify_small(b)
            ref, ref_tally = sh.p.verify_batch(b)
            assert got == ref, (n, [i for i in range(n) if got[i] != ref[i]][:8])
            assert tally == ref_tally, n
            check = sorted(bad | (set(range(n)) if n <= 256 else set(rnd.sample(range(n), 60))))
            sub = b"".join(b[i * sh.size : (i + 1) * sh.size] for i in check)
            want = sh.op.verify_batch(sub, threads=16)
            assert [got[i] for i in check] == want, n
            assert all(got[i] != 0 for i in bad), n
            if n <= 256:
                assert tally == sh.op.tally(b, want), n
            seen |= set(got)
        kinds = {s & 0xFF for s in seen}
        assert {0, eg.BAD_POINT, eg.BAD_SCALAR} <= kinds
        if kind == "qv":
            assert {eg.QV_VARIANT_CHALLENGE | (k << 8) for k in range(n_options)} <= seen
            assert {eg.QV_CREDIT_RANGE_CHALLENGE, eg.QV_CREDIT_EQUIV_CHALLENGE} <= seen
        else:
            assert eg.RANGE_CHALLENGE in kinds and ((eg.SUM_CHALLENGE in kinds) == (kind == "single"))
        pts, scs = sh.classify_items(oracle, pool[: sh.size])
        for it in (pts[0], pts[len(pts) // 2], pts[-1]):
            assert (eg.BAD_POINT | (it << 8)) in seen
        for it in (scs[0], scs[len(scs) // 2], scs[-1]):
            assert (eg.BAD_SCALAR | (it << 8)) in seen
    finally:
        sh.close()


# ------------------------------------------------------------------ the reference's snapshots
def test_reference_snapshots_and_their_tampered_twins(eg, ctx, oracle, golden, pk):
    cases = [(eg.ChoiceParams(ctx, pk, 5, True), oracle.ChoiceParams(pk, 5, True), "encrypted-choice"),
             (eg.ChoiceParams(ctx, pk, 5, False), oracle.ChoiceParams(pk, 5, False), "encrypted-multi-choice"),
             (eg.QuadraticVotingParams(ctx, pk, 5, 15), oracle.QvParams(pk, 5, 15), "qv-ballot")]
    for p, op, name in cases:
        ballot = bytes.fromhex(golden[name]["packed"])
        st, tally = p.verify_small(ballot)
        assert st == [0] == op.verify_batch(ballot), name
        assert tally == op.tally(ballot, [0]) == p.verify_batch(ballot)[1], name
        twins = [E.tamper(ballot, s) for s in range(12)] + [E.tamper(ballot, 100 + it, it) for it in range(0, len(ballot) // 32, 3)]
        raw = b"".join(twins)
        got, tally = p.verify_small(raw)
        want = op.verify_batch(raw)
        assert got == want and all(w != 0 for w in want), name
        assert tally == op.tally(raw, want)
        assert len({w & 0xFF for w in want}) >= 2, name          # a multi-choice ballot has no sum proof: bad point and range challenge
        p.close()


# ------------------------------------------------------------------ the edge corpus
@pytest.mark.parametrize("fam_name", ["single2", "single5", "single16", "multi3of16", "multi20", "qv5x20"])
def test_edge_corpus_through_the_small_path(eg, ctx, fam_name):
    """nonce 0, r in {0, 1, l - 1}, cancelling slots, keys G / -G / [2]G and the comb-digit corners: verdicts and tallies equal the
    oracle's, and each case has its rejected twin"""
    for key_name in E.KEY_NAMES:
        fam = E.family(fam_name, key_name)
        p = fam.gpu_params(eg, ctx)
        try:
            batch = []
            for i, e in enumerate(fam.edges):
                batch += [e.ballot, E.tamper(e.ballot, i, fam.challenge_item), E.tamper(e.ballot, 1000 + i)]
            want = [fam.verify(b) for b in batch]
            assert all(w == 0 for w in want[0::3]) and all(w != 0 for w in want[1::3]), key_name
            for lo in range(0, len(batch), 4096):
                raw = b"".join(batch[lo : lo + 4096])
                got, tally = p.verify_small(raw)
                assert got == want[lo : lo + 4096], key_name
                assert tally == fam.tally(raw, got), key_name
            pair = [e.ballot for e in fam.edges if e.name.startswith("cancel_")]
            raw = b"".join(pair + [E.tamper(pair[0], 5, fam.challenge_item)])
            got, tally = p.verify_small(raw)
            assert got[:2] == [0, 0] and got[2] != 0
            assert all(tally[64 * k : 64 * k + 32] == E.IDENTITY for k in range(fam.n_options))
        finally:
            p.close()


def test_small_path_on_the_ring_group_walk(eg, ctx, monkeypatch):
    """a plan built for the ring-group walk (tables of one group of rings at a time): the small path walks it as the batch path does"""
    for group in ("1", "2"):
        monkeypatch.setenv("EG_RING_GROUP", group)
        for name in ("single5", "multi20"):
            fam = E.family(name, "golden")
            assert eg.plan_describe(fam.kind, fam.n_options)["ring_group"] == int(group)
            p = fam.gpu_params(eg, ctx)
            try:
                batch = []
                for i, e in enumerate(fam.edges[:40]):
                    batch += [e.ballot, E.tamper(e.ballot, i, fam.challenge_item)]
                raw = b"".join(batch) + fam.random_ballots(99, 30)
                want = [fam.verify(raw[i : i + fam.size]) for i in range(0, len(raw), fam.size)]
                got, tally = p.verify_small(raw)
                assert got == want and tally == fam.tally(raw, want)
                assert p.verify_batch(raw) == (got, tally)
            finally:
                p.close()


# ------------------------------------------------------------------ tally semantics
@pytest.mark.parametrize("kind", ["single", "qv"])
def test_running_tally_over_interleaved_small_and_batch_calls(eg, ctx, oracle, pk, kind):
    op = oracle.QvParams(pk, 5, 20) if kind == "qv" else oracle.ChoiceParams(pk, 5, True)
    p = eg.QuadraticVotingParams(ctx, pk, 5, 20) if kind == "qv" else eg.ChoiceParams(ctx, pk, 5, True)
    sz = op.ballot_size
    raw = bytearray(op.generate_batch(2024, 0, 200, threads=8))
    for i in range(0, 200, 9):
        raw[i * sz + 40] ^= 2
    raw = bytes(raw)
    want = op.verify_batch(raw, threads=8)
    cuts = [0, 1, 3, 70, 71, 135, 200]
    for k in range(len(cuts) - 1):
        part = raw[cuts[k] * sz : cuts[k + 1] * sz]
        st, t = (p.verify_small if k % 2 == 0 else p.verify_batch)(part)
        assert st == want[cuts[k] : cuts[k + 1]]
        assert t == op.tally(part, st)                           # tally_out: this call's batch alone
    assert p.tally_encode() == op.tally(raw, want)               # the running tally: every accepted ballot of every call
    st, t = p.verify_small(raw[: 10 * sz], with_tally=False)     # with_tally=False returns nothing and still accumulates
    assert t is None and st == want[:10]
    both = raw + raw[: 10 * sz]
    assert p.tally_encode() == op.tally(both, want + want[:10])
    snapshot = p.tally_encode()
    p.tally_reset()
    assert p.tally_encode() == op.tally(b"", [])
    p.tally_add(snapshot)
    p.verify_small(raw[: 5 * sz])
    assert p.tally_encode() == op.tally(both + raw[: 5 * sz], want + want[:10] + want[:5])
    p.close()


# ------------------------------------------------------------------ entry forms
def test_entry_forms(eg, ctx, oracle, pk, torch):
    op = oracle.ChoiceParams(pk, 5, True)
    p = eg.ChoiceParams(ctx, pk, 5, True)
    sz = op.ballot_size
    raw = bytearray(op.generate_batch(808, 0, 300, threads=8))
    for i in range(0, 300, 7):
        raw[i * sz + 330] ^= 1
    raw = bytes(raw)
    want = op.verify_batch(raw, threads=8)
    # host and device forms agree
    host, _ = p.verify_small(raw)
    d = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    st = torch.full((300,), -1, dtype=torch.int32, device="cuda")
    p.tally_reset()
    p.verify_small_device(300, d.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert st.tolist() == host == want
    assert p.tally_encode() == op.tally(raw, want)
    # a non-null stream orders the call behind earlier work on that stream: the ballots are written by a copy enqueued on it
    s = torch.cuda.Stream()
    src = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
    with torch.cuda.stream(s):
        big = torch.empty(1 << 26, dtype=torch.float32, device="cuda").normal_()       # keeps the stream busy first
        big.mul_(2.0).add_(1.0)
        d2 = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
        d2.copy_(src, non_blocking=True)
        st2 = torch.full((300,), -1, dtype=torch.int32, device="cuda")
        p.verify_small_device(300, d2.data_ptr(), st2.data_ptr(), stream=s.cuda_stream)
        after = st2.clone()                                                           # ... and later work on it sees the verdicts
    s.synchronize()
    assert after.tolist() == want
    # n = 0 is accepted, n = SMALL_BATCH_MAX + 1 refused (and changes nothing)
    assert p.verify_small(b"") == ([], op.tally(b"", []))
    p.verify_small_device(0, 0, 0)
    before = p.tally_encode()
    too_many = torch.zeros((eg.SMALL_BATCH_MAX + 1) * sz, dtype=torch.uint8, device="cuda")
    st3 = torch.zeros(eg.SMALL_BATCH_MAX + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(eg.EgError, match="EG_SMALL_BATCH_MAX"):
        p.verify_small_device(eg.SMALL_BATCH_MAX + 1, too_many.data_ptr(), st3.data_ptr())
    with pytest.raises(eg.EgError):
        p.verify_small(bytes((eg.SMALL_BATCH_MAX + 1) * sz))
    assert p.tally_encode() == before
    full = op.generate_batch(5, 0, 16, threads=8) * (eg.SMALL_BATCH_MAX // 16)          # exactly the maximum is taken
    assert p.verify_small(full)[0] == [0] * eg.SMALL_BATCH_MAX
    # refused while a JSON stream is open on the object
    stream = p.json_stream()
    with pytest.raises(eg.EgError, match="JSON stream"):
        p.verify_small(raw[:sz])
    with pytest.raises(eg.EgError, match="JSON stream"):
        p.verify_small_device(1, d.data_ptr(), st.data_ptr())
    stream.abort()
    assert p.verify_small(raw[:sz])[0] == want[:1]
    p.close()


# ------------------------------------------------------------------ concurrency with the batch path
def test_small_calls_beside_large_batch_calls_on_one_context(eg, ctx, oracle, pk, torch):
    """two threads, two params objects of one context, two hundred calls each: one makes small calls (host form and device form on a
    stream of its own, in turn), the other batch calls of 2^17 ballots on its stream, so that small calls are enqueued while a batch call
    is on the GPU; every verdict and both tallies equal the serial result"""
    op = oracle.ChoiceParams(pk, 5, True)
    a, b = eg.ChoiceParams(ctx, pk, 5, True), eg.ChoiceParams(ctx, pk, 5, True)
    sz = a.ballot_size
    big_n, calls_big, calls_small = 1 << 17, 200, 200
    big = torch.zeros(big_n * sz, dtype=torch.uint8, device="cuda")
    b.encrypt_batch_device(999, 0, big_n, big.data_ptr())
    ctx.synchronize()
    for i in range(0, big_n, 1001):
        big[i * sz + 321] ^= 1
    small_raw = bytearray(op.generate_batch(4, 0, 40, threads=8))
    for i in range(0, 40, 6):
        small_raw[i * sz + 50] ^= 8
    small_raw = bytes(small_raw)
    want_small = op.verify_batch(small_raw, threads=8)
    d_small = torch.frombuffer(bytearray(small_raw), dtype=torch.uint8).cuda()
    # the serial result
    st_big = torch.zeros(big_n, dtype=torch.int32, device="cuda")
    b.verify_batch_device(big_n, big.data_ptr(), st_big.data_ptr())
    torch.cuda.synchronize()
    serial_big = st_big.clone()
    one_big_tally = b.tally_encode()
    assert int((serial_big != 0).sum()) == len(range(0, big_n, 1001))
    b.tally_reset()
    results, errors, big_done, overlapped = [], [], threading.Event(), [0]

    def small_worker():
        try:
            rnd = random.Random(1)
            s = torch.cuda.Stream()
            for k in range(calls_small):
                lo = rnd.randrange(0, 36)
                hi = lo + rnd.randrange(1, 5)
                if k % 2:
                    st, _ = a.verify_small(small_raw[lo * sz : hi * sz])
                else:
                    with torch.cuda.stream(s):
                        out = torch.full((hi - lo,), -1, dtype=torch.int32, device="cuda")
                        a.verify_small_device(hi - lo, d_small.data_ptr() + lo * sz, out.data_ptr(), stream=s.cuda_stream)
                    s.synchronize()
                    st = out.tolist()
                overlapped[0] += not big_done.is_set()
                results.append((lo, hi, st))
        except Exception as e:          # noqa: BLE001
            errors.append(e)

    def big_worker():
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(calls_big):
                    out = torch.zeros(big_n, dtype=torch.int32, device="cuda")
                    b.verify_batch_device(big_n, big.data_ptr(), out.data_ptr(), stream=s.cuda_stream)
                    same = (out == serial_big).all()
                    s.synchronize()
                    if not bool(same):
                        errors.append(AssertionError("batch verdicts differ beside small calls"))
        except Exception as e:          # noqa: BLE001
            errors.append(e)
        finally:
            big_done.set()

    ts = [threading.Thread(target=small_worker), threading.Thread(target=big_worker)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert len(results) == calls_small
    print(f"{overlapped[0]} of {calls_small} small calls returned while the batch thread was still calling")
    assert overlapped[0] > 0, "no small call ran beside a batch call"
    accepted = b""
    for lo, hi, st in results:
        assert st == want_small[lo:hi]
        accepted += b"".join(small_raw[i * sz : (i + 1) * sz] for i in range(lo, hi) if want_small[i] == 0)
    assert a.tally_encode() == op.tally(accepted, [0] * (len(accepted) // sz))
    grp = eg.Ristretto(ctx)
    acc = op.tally(b"", [])
    for _ in range(calls_big):
        acc, ok = grp.element_add(acc, one_big_tally)
    assert b.tally_encode() == acc
    a.close(); b.close()


# ------------------------------------------------------------------ the latency relation
def _median_ms(torch, fn, n, d, st):
    for _ in range(3):
        fn(n, d.data_ptr(), st.data_ptr()); torch.cuda.synchronize()
    ts = []
    for _ in range(21):
        t0 = time.perf_counter()
        fn(n, d.data_ptr(), st.data_ptr()); torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


@pytest.mark.parametrize("kind,sizes", [("single", (1, 64, 256)), ("qv", (1, 64))])
def test_small_entry_is_faster_than_the_batch_entry(eg, ctx, pk, torch, kind, sizes):
    """median of 21 timed call + synchronize on device-resident ballots after 3 warm-up calls, both entries in this process on the same
    chip at the same clock: the small entry must beat the batch entry (no margin beyond the medians; no absolute milliseconds)"""
    p = eg.QuadraticVotingParams(ctx, pk, 5, 20) if kind == "qv" else eg.ChoiceParams(ctx, pk, 5, True)
    n_max = max(sizes)
    d = torch.zeros(n_max * p.ballot_size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(77, 0, n_max, d.data_ptr())
    ctx.synchronize()
    sa = torch.zeros(n_max, dtype=torch.int32, device="cuda")
    sb = torch.ones(n_max, dtype=torch.int32, device="cuda")
    for n in sizes:
        batch = _median_ms(torch, p.verify_batch_device, n, d, sa)
        small = _median_ms(torch, p.verify_small_device, n, d, sb)
        print(f"{kind} n = {n}: batch {batch:.3f} ms, small {small:.3f} ms, ratio {small / batch:.2f}")
        assert bool((sb[:n] == 0).all()) and bool((sa[:n] == 0).all())
        assert small < batch, (kind, n, small, batch)
    p.close()
