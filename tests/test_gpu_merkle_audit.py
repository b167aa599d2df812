"""The receipt log's audit entries (eg_merkle_heads / _consistency / _consistency_check and their _device forms) on the GPU: the heads
the log had at earlier sizes, consistency proofs out of the node store and the check of many of them.  Every expected value comes from
the pure-Python model tests/merkle_audit_ref.py (hashlib, written from the text of RFC 9162 2.1.4); heads, proof rows and lengths are
compared byte for byte, verdicts and found words exactly, with canaries behind every array the library writes."""
import random
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import merkle_audit_ref as A
import merkle_ref as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CANARY = 0x5C
PAD = 64
BIG = (1 << 20) + 3


@pytest.fixture(scope="module")
def eg():
    import elastic_elgamal_amd as m

    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


@pytest.fixture(scope="module")
def ctx(eg):
    c = eg.Context(0)
    yield c
    c.close()


def dev(torch, data: bytes, pad=PAD):
    """device bytes with a canary tail"""
    a = np.full(len(data) + pad, CANARY, dtype=np.uint8)
    a[: len(data)] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(a).cuda()


def room(torch, size, pad=PAD):
    return torch.full((size + pad,), CANARY, dtype=torch.uint8, device="cuda")


def host(t, size=None):
    b = t.cpu().numpy().tobytes()
    return b if size is None else b[:size]


def tail_ok(t, size, pad=PAD):
    return host(t)[size:] == bytes([CANARY]) * pad


def u64s(values):
    return np.asarray(values, dtype=np.uint64).tobytes()


def u32s(values):
    return np.asarray(values, dtype=np.uint32).tobytes()


def leaves_of(n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, n * 32, dtype=np.uint8).tobytes()
    return raw, [raw[32 * i:32 * i + 32] for i in range(n)]


_trees = {}


def model_tree(n, seed=5):
    """(raw log, leaves, root, levels) of the model, computed once per size and left unchanged"""
    if (n, seed) not in _trees:
        raw, leaves = leaves_of(n, seed)
        levels = M.levels(leaves)
        root = levels[-1][0] if n else M.mth([])
        if n <= 4096:
            assert root == M.mth(leaves)                                  # the recursion of the RFC
        _trees[n, seed] = (raw, leaves, root, levels)
    return _trees[n, seed]


def tree_dev(torch, eg, ctx, raw, n, stream=0):
    """the log and its node store on the device, built by the library -> (root, d_log, d_nodes, node store bytes)"""
    rl = eg.ReceiptLog(ctx)
    d_log, d_root = dev(torch, raw), room(torch, 32)
    size = rl.nodes_bytes(n)
    d_nodes = room(torch, size)
    torch.cuda.synchronize()
    rl.tree_device(n, d_log.data_ptr(), d_root.data_ptr(), d_nodes.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert tail_ok(d_nodes, size) and tail_ok(d_root, 32)
    return host(d_root, 32), d_log, d_nodes, host(d_nodes, size)


def audit_dev(torch, eg, ctx, olds, n, d_log, d_nodes, root, stream=0):
    """heads_device, consistency_device and consistency_check_device (of the heads and proofs as issued) for the old sizes
    -> (heads, found of the heads, proof rows, proof_len, verdicts, found)"""
    rl = eg.ReceiptLog(ctx)
    m, row = len(olds), 32 * (rl.depth(n) + 1)
    d_old = dev(torch, u64s(olds))
    d_heads, d_hfound = room(torch, 32 * m), dev(torch, u32s([77]))
    d_proofs, d_len = room(torch, m * row), room(torch, 4 * m)
    d_root = dev(torch, root)
    d_verdict, d_found = room(torch, 4 * m), dev(torch, u32s([77, 77, 77, 77]))
    torch.cuda.synchronize()
    rl.heads_device(m, d_old.data_ptr(), n, d_log.data_ptr(), d_nodes.data_ptr(), d_heads.data_ptr(), d_hfound.data_ptr(), stream)
    rl.consistency_device(m, d_old.data_ptr(), n, d_log.data_ptr(), d_nodes.data_ptr(), d_proofs.data_ptr(), d_len.data_ptr(), stream)
    rl.consistency_check_device(m, d_old.data_ptr(), d_heads.data_ptr(), d_proofs.data_ptr(), row, d_len.data_ptr(), n, d_root.data_ptr(),
                                d_verdict.data_ptr(), d_found.data_ptr(), stream)
    torch.cuda.synchronize()
    assert tail_ok(d_heads, 32 * m) and tail_ok(d_hfound, 4) and tail_ok(d_proofs, m * row) and tail_ok(d_len, 4 * m)
    assert tail_ok(d_verdict, 4 * m) and tail_ok(d_found, 16) and tail_ok(d_old, 8 * m)
    heads, rows = host(d_heads, 32 * m), host(d_proofs, m * row)
    return ([heads[32 * j:32 * j + 32] for j in range(m)], np.frombuffer(host(d_hfound, 4), dtype=np.uint32).tolist(),
            [rows[j * row:(j + 1) * row] for j in range(m)], np.frombuffer(host(d_len, 4 * m), dtype=np.uint32).tolist(),
            np.frombuffer(host(d_verdict, 4 * m), dtype=np.uint32).tolist(), np.frombuffer(host(d_found, 16), dtype=np.uint32).tolist())


# ------------------------------------------------------------------ every old size of small logs
@pytest.mark.parametrize("n", [1, 2, 3, 6, 7, 8, 64, 65])
def test_heads_proofs_and_checks_of_every_old_size(torch, eg, ctx, n):
    raw, leaves, root, _ = model_tree(n)
    got_root, d_log, d_nodes, store = tree_dev(torch, eg, ctx, raw, n)
    assert got_root == root
    olds = list(range(n + 2))                                             # 0 and N + 1 among them
    heads, hfound, rows, lens, verdict, found = audit_dev(torch, eg, ctx, olds, n, d_log, d_nodes, root)
    d = M.depth(n)
    assert heads[0] == M.H(b"") and heads[n + 1] == bytes(32) and hfound == [1] and heads[n] == root
    for m in range(1, n + 1):
        assert heads[m] == M.mth(leaves[:m]), m                          # MTH of the prefix, by the RFC's recursion
        want = A.proof(m, leaves)                                         # PROOF(m, D[N]), by the RFC's recursion
        assert lens[m] == len(want) == A.consistency_len(m, n) and rows[m] == b"".join(want) + bytes(32 * (d + 1 - len(want))), m
        assert A.check(m, n, heads[m], want, root) == 0
    assert lens[0] == lens[n + 1] == M.NO_PATH and rows[0] == rows[n + 1] == bytes(32 * (d + 1))
    assert verdict == [A.BAD_INDEX] + [0] * n + [A.BAD_INDEX] and found == [2, 0, 0, 0]
    # the host forms say the same
    rl = eg.ReceiptLog(ctx)
    assert rl.heads(olds, raw, store) == (heads, [1])
    proofs, raw_rows, host_lens = rl.consistency(olds, raw, store)
    assert raw_rows == b"".join(rows) and host_lens == lens and proofs[0] is None and proofs[n + 1] is None
    assert rl.consistency_check(olds[1:n + 1], heads[1:n + 1], proofs[1:n + 1], n, root) == ([0] * n, [0, 0, 0, 0])


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_the_tile_seams_and_the_switch_to_no_seed(torch, eg, ctx, n):
    raw, leaves, root, _ = model_tree(n)
    got_root, d_log, d_nodes, _ = tree_dev(torch, eg, ctx, raw, n)
    assert got_root == root
    olds = [m for m in (1, 2, 511, 512, 513, 1023, 1024, 1025, n - 1, n) if m <= n]
    heads, hfound, rows, lens, verdict, found = audit_dev(torch, eg, ctx, olds, n, d_log, d_nodes, root)
    d = M.depth(n)
    for j, m in enumerate(olds):
        want = A.proof(m, leaves)
        assert heads[j] == M.mth(leaves[:m]), m
        assert lens[j] == len(want) == A.consistency_len(m, n) and rows[j] == b"".join(want) + bytes(32 * (d + 1 - len(want))), m
        assert A.check(m, n, heads[j], want, root) == 0, m
    assert verdict == [0] * len(olds) and found == [0, 0, 0, 0] and hfound == [0]


def test_a_log_that_needs_the_third_launch(torch, eg, ctx):
    """2^20 + 3 leaves: proofs that walk the levels of all three launches of the tree; the longest rows fill all 22 entries"""
    n = BIG
    raw, leaves, root, levels = model_tree(n)
    got_root, d_log, d_nodes, _ = tree_dev(torch, eg, ctx, raw, n)
    assert got_root == root and M.depth(n) == 21
    olds = [1, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, n - 1, n]
    heads, hfound, rows, lens, verdict, found = audit_dev(torch, eg, ctx, olds, n, d_log, d_nodes, root)
    for j, m in enumerate(olds):
        want = A.store_proof(m, levels)                                   # equal to the recursion: the model's self-check
        assert lens[j] == len(want) == A.consistency_len(m, n) <= 22 and rows[j] == b"".join(want) + bytes(32 * (22 - len(want))), m
        assert heads[j] == A.past_head(m, levels), m
        assert A.check(m, n, heads[j], want, root) == 0, m                # the literal algorithm of RFC 9162 2.1.4.2 accepts head and proof
        if m <= 1025:
            assert heads[j] == M.mth(leaves[:m]), m
    # old size 1023 = ..1111111111 has its seed at level 0 and a sibling at every one of the 21 levels: the bound depth(N) + 1 is reached
    assert heads[5] == levels[20][0] and heads[8] == root and max(lens) == lens[1] == 22 and lens[5] == 1 and lens[8] == 0
    assert verdict == [0] * len(olds) and found == [0, 0, 0, 0] and hfound == [0]


# ------------------------------------------------------------------ forgeries
KINDS = ("zero", "above", "short", "long", "seed", "last", "old_root", "other")


def test_a_wavefront_of_forged_proofs_among_good_ones(torch, eg, ctx):
    """257 proofs against a 777-leaf log: forgeries at lanes 0, 63, 64 and last and a whole wavefront (lanes 128 .. 191) of them, of eight
    kinds; every verdict and all four found words against the model.  The rows of proofs with a wrong length are never read: they lie
    with a stride that leaves room for the longer length."""
    n, count = 777, 257
    raw, leaves, root, levels = model_tree(n)
    rng = random.Random(9)
    rl = eg.ReceiptLog(ctx)
    d = M.depth(n)
    stride = 32 * (d + 2)
    seeded = [m for m in range(3, n) if m & (m - 1)]                      # below N and no power of two: a proof with a seed
    olds = [rng.choice(seeded) for _ in range(count)]
    olds[5], olds[6], olds[7], olds[8] = n, 512, 1, n - 1                 # good ones: the empty proof, no seed, the ragged edge
    recs = [[m, A.past_head(m, levels), A.store_proof(m, levels)] for m in olds]
    assert all(r[1] == M.mth(leaves[:r[0]]) and r[2] == A.proof(r[0], leaves) for r in recs[:12])
    forged = {0: "seed", 63: "old_root", 64: "zero", count - 1: "short"}
    for lane in range(128, 192):
        forged[lane] = KINDS[lane % 8]
    for lane, kind in forged.items():
        r = recs[lane]
        if kind == "zero":
            r[0] = 0
        elif kind == "above":
            r[0] = n + 1
        elif kind == "short":
            r[2] = r[2][:-1]
        elif kind == "long":
            r[2] = r[2] + [bytes(32)]
        elif kind == "seed":
            r[2] = [A.flip(r[2][0], lane)] + r[2][1:]
        elif kind == "last":
            r[2] = r[2][:-1] + [A.flip(r[2][-1], 255 - lane)]
        elif kind == "old_root":
            r[1] = A.flip(r[1], lane)
        elif kind == "other":
            other = next(m for m in seeded if m != r[0] and A.consistency_len(m, n) == len(r[2])) if lane % 16 == 7 else r[0] + 1
            r[2] = A.store_proof(other, levels)                           # another size's proof: of the same length, or judged by it
    want = [A.check(m, n, old_root, proof, root) for m, old_root, proof in recs]
    assert [want[k] for k in (0, 63, 64, count - 1)] == [A.MISMATCH_OLD, A.MISMATCH_OLD, A.BAD_INDEX, A.BAD_LENGTH]
    assert all(want[k] for k in forged) and sum(1 for w in want if w == 0) == count - len(forged)
    assert {A.BAD_INDEX, A.BAD_LENGTH, A.MISMATCH, A.MISMATCH_OLD} <= set(want[128:192])
    verdict, found = rl.consistency_check([r[0] for r in recs], [r[1] for r in recs], b"".join(b"".join(r[2]) + bytes(stride - 32 * len(r[2])) for r in recs), n,
                                          root, proof_len=[len(r[2]) for r in recs], proof_stride=stride)
    assert verdict == want and found == [want.count(1), want.count(2), want.count(3), want.count(4)]
    # against the root of another tree nothing is proven; the proofs that gave their old head still do
    other = model_tree(1025)[2]
    verdict, found = rl.consistency_check([r[0] for r in recs], [r[1] for r in recs], [b"".join(r[2]) for r in recs], n, other)
    assert all(verdict) and found[2] == sum(1 for w in want if w in (0, A.MISMATCH)) and found[3] == want.count(A.MISMATCH_OLD)


def test_a_forked_log_is_told_from_a_grown_one(torch, eg, ctx):
    """the same leaves with one leaf below m replaced: the fork's proof for m does not give the honest old head, and the honest proof does
    not give the fork's root"""
    n, m = 300, 150
    raw, leaves, root, levels = model_tree(n)
    forked = leaves[:70] + [M.H(b"rewritten")] + leaves[71:]
    rl = eg.ReceiptLog(ctx)
    fork_raw = b"".join(forked)
    fork_root, fork_store = rl.tree(fork_raw)
    honest_root, store = rl.tree(raw)
    assert honest_root == root and fork_root == M.mth(forked) != root
    head_m = rl.heads([m], raw, store)[0][0]
    assert head_m == M.mth(leaves[:m]) != rl.heads([m], fork_raw, fork_store)[0][0]
    honest, fork = rl.consistency([m], raw, store)[0][0], rl.consistency([m], fork_raw, fork_store)[0][0]
    assert honest == b"".join(A.proof(m, leaves)) and fork == b"".join(A.proof(m, forked))
    verdict, found = rl.consistency_check([m, m, m], [head_m] * 3, [honest, fork, honest], n, root)
    assert verdict == [0, A.MISMATCH_OLD, 0] and found == [0, 0, 0, 1]
    verdict, found = rl.consistency_check([m, m], [head_m] * 2, [fork, honest], n, fork_root)
    assert verdict == [A.MISMATCH_OLD, A.MISMATCH] and found == [0, 0, 1, 1]
    assert verdict == [A.check(m, n, head_m, A.proof(m, forked), fork_root), A.check(m, n, head_m, A.proof(m, leaves), fork_root)]


# ------------------------------------------------------------------ the entry forms
def test_entry_forms_agree_on_a_caller_stream(torch, eg, ctx):
    n = 1500
    raw, leaves, root, levels = model_tree(n, seed=8)
    s = torch.cuda.Stream()
    got_root, d_log, d_nodes, store = tree_dev(torch, eg, ctx, raw, n, stream=s.cuda_stream)
    assert got_root == root
    olds = list(range(1, n + 1, 13)) + [n, 0, n + 1, 1 << 40]
    heads, hfound, rows, lens, verdict, found = audit_dev(torch, eg, ctx, olds, n, d_log, d_nodes, root, stream=s.cuda_stream)
    rl = eg.ReceiptLog(ctx)
    assert rl.heads(olds, raw, store) == (heads, hfound) and hfound == [2]
    proofs, raw_rows, host_lens = rl.consistency(olds, raw, store)
    assert raw_rows == b"".join(rows) and host_lens == lens
    assert rl.consistency_check(olds, heads, raw_rows, n, root, proof_len=[0 if x == M.NO_PATH else x for x in lens],
                                proof_stride=32 * (M.depth(n) + 1)) == (verdict, found)
    assert verdict == [0] * (len(olds) - 3) + [A.BAD_INDEX] * 3 and found == [3, 0, 0, 0]
    assert all(heads[j] == A.past_head(m, levels) and proofs[j] == b"".join(A.store_proof(m, levels)) for j, m in enumerate(olds[:-3]))


def test_m_zero(torch, eg, ctx):
    rl = eg.ReceiptLog(ctx)
    raw, leaves, root, _ = model_tree(5)
    store = rl.tree(raw)[1]
    assert rl.heads([], raw, store) == ([], [0]) and rl.consistency([], raw, store) == ([], b"", [])
    assert rl.consistency_check([], [], [], 5, root) == ([], [0, 0, 0, 0])
    assert rl.heads([0], b"", b"") == ([M.H(b"")], [0]) and rl.heads([1], b"", b"") == ([bytes(32)], [1])        # the empty log
    d_found, d_hfound = dev(torch, u32s([7, 7, 7, 7])), dev(torch, u32s([7]))
    rl.consistency_check_device(0, 0, 0, 0, 128, 0, 5, 0, 0, d_found.data_ptr())
    rl.heads_device(0, 0, 5, 0, 0, 0, d_hfound.data_ptr())
    rl.heads_device(0, 0, 5, 0, 0, 0, 0)
    rl.consistency_device(0, 0, 5, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert host(d_found, 16) == u32s([0, 0, 0, 0]) and tail_ok(d_found, 16) and host(d_hfound, 4) == u32s([0]) and tail_ok(d_hfound, 4)


def test_every_refusal_with_a_live_context(torch, eg, ctx):
    rl = eg.ReceiptLog(ctx)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    b = buf.data_ptr()
    big = 1 << 31

    def refused(text, fn, *args, **kw):
        with pytest.raises(eg.EgError, match=text):
            fn(*args, **kw)

    refused("m is 2\\^31 or more", rl.heads_device, big, b, 5, b, b, b, b)
    refused("N is 2\\^31 or more", rl.heads_device, 1, b, big, b, b, b, b)
    for k in (1, 5, 6):
        args = [1, b, 5, b, b, b, b]
        args[k] = 0
        refused("null size, heads or found", rl.heads_device, *args)
    refused("null log or nodes", rl.heads_device, 1, b, 5, 0, b, b, b)
    refused("null log or nodes", rl.heads_device, 1, b, 5, b, 0, b, b)
    refused("8-byte aligned", rl.heads_device, 1, b + 4, 5, b, b, b, b)
    for k in (3, 4, 5, 6):
        args = [1, b, 5, b, b, b, b]
        args[k] = b + 2
        refused("4-byte aligned", rl.heads_device, *args)
    refused("m is 2\\^31 or more", rl.consistency_device, big, b, 5, b, b, b, b)
    refused("N is 2\\^31 or more", rl.consistency_device, 1, b, big, b, b, b, b)
    for k in (1, 5, 6):
        args = [1, b, 5, b, b, b, b]
        args[k] = 0
        refused("null old_size, proofs or proof_len", rl.consistency_device, *args)
    refused("null log or nodes", rl.consistency_device, 1, b, 5, 0, b, b, b)
    refused("null log or nodes", rl.consistency_device, 1, b, 5, b, 0, b, b)
    refused("8-byte aligned", rl.consistency_device, 1, b + 4, 5, b, b, b, b)
    for k in (3, 4, 5, 6):
        args = [1, b, 5, b, b, b, b]
        args[k] = b + 2
        refused("4-byte aligned", rl.consistency_device, *args)
    refused("m is 2\\^31 or more", rl.consistency_check_device, big, b, b, b, 128, b, 5, b, b, b)
    refused("N is 2\\^31 or more", rl.consistency_check_device, 1, b, b, b, 1024, b, big, b, b, b)
    refused("proof_stride is below 32 \\* \\(depth\\(N\\) \\+ 1\\)", rl.consistency_check_device, 1, b, b, b, 127, b, 5, b, b, b)
    refused("proof_stride is below 32 \\* \\(depth\\(N\\) \\+ 1\\)", rl.consistency_check_device, 1, b, b, b, 96, b, 5, b, b, b)
    refused("proof_stride is no multiple of 4", rl.consistency_check_device, 1, b, b, b, 130, b, 5, b, b, b)
    refused("null proofs", rl.consistency_check_device, 1, b, b, 0, 128, b, 5, b, b, b)
    for k in (1, 2, 5, 7, 8, 9):
        args = [1, b, b, b, 128, b, 5, b, b, b]
        args[k] = 0
        refused("null old_size, old_root, proof_len, root, verdict or found", rl.consistency_check_device, *args)
    refused("8-byte aligned", rl.consistency_check_device, 1, b + 4, b, b, 128, b, 5, b, b, b)
    for k in (2, 3, 5, 7, 8, 9):
        args = [1, b, b, b, 128, b, 5, b, b, b]
        args[k] = b + 2
        refused("4-byte aligned", rl.consistency_check_device, *args)
    torch.cuda.synchronize()
    assert int(buf.sum().item()) == 0                                          # nothing was launched


# ------------------------------------------------------------------ beside the verifier, and end to end
@pytest.fixture(scope="module")
def election(eg, ctx, oracle):
    pk = oracle.keypair_from_seed(12345)[1]
    return eg.ChoiceParams(ctx, pk, 5, True)


def test_a_pass_beside_a_verifying_thread(torch, eg, ctx, election):
    """two threads derive heads, issue and check proofs on streams of their own while a third verifies ballots on the same context: the
    entries take no lock and use no workspace of the context"""
    p = election
    n_ballots = 1500
    d_msgs = room(torch, n_ballots * p.ballot_size)
    p.encrypt_batch_device(808, 0, n_ballots, d_msgs.data_ptr())
    p.ctx.synchronize()
    n = 1500
    raw, leaves, root, levels = model_tree(n, seed=8)
    _, d_log, d_nodes, _ = tree_dev(torch, eg, ctx, raw, n)
    olds = list(range(1, n + 1, 7)) + [n + 1]
    want_heads = [A.past_head(m, levels) for m in olds[:-1]] + [bytes(32)]
    want_rows = [b"".join(A.store_proof(m, levels)) for m in olds[:-1]] + [b""]
    errors, results = [], {}

    def worker(k):
        try:
            s = torch.cuda.Stream()
            results[k] = [audit_dev(torch, eg, ctx, olds, n, d_log, d_nodes, root, stream=s.cuda_stream) for _ in range(3)]
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    def verifier():
        try:
            s = torch.cuda.Stream()
            st = torch.full((n_ballots,), 9, dtype=torch.int32, device="cuda")
            for _ in range(3):
                p.verify_batch_device(n_ballots, d_msgs.data_ptr(), st.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            results["status"] = st.cpu().tolist()
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(0,)), threading.Thread(target=worker, args=(1,)), threading.Thread(target=verifier)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    p.tally_reset()
    assert not errors, errors
    assert results["status"] == [0] * n_ballots
    row = 32 * (M.depth(n) + 1)
    for k in (0, 1):
        for heads, hfound, rows, lens, verdict, found in results[k]:
            assert heads == want_heads and hfound == [1] and rows == [r + bytes(row - len(r)) for r in want_rows]
            assert verdict == [0] * (len(olds) - 1) + [A.BAD_INDEX] and found == [1, 0, 0, 0] and lens[-1] == M.NO_PATH


def test_end_to_end_a_kept_head_and_a_receipt_without_re_issue(torch, eg, ctx, election):
    """two batches of generated ballots through verify -> weed -> leaves -> tree.  The head after batch one is kept; the final store gives
    it back, its consistency proof against the final head is proven, and a batch-one receipt still proves against the kept head."""
    p = election
    size = p.ballot_size
    fresh = p.encrypt_batch(4141, 0, 260)
    rl = eg.ReceiptLog(ctx, b"election-20")
    log, board, kept = b"", b"", None
    for batch in (fresh[:150 * size], fresh[150 * size:]):
        n = len(batch) // size
        status, _ = p.verify_batch(batch)
        p.tally_reset()
        assert status == [0] * n
        dup, weeded, appended = p.weed(batch, status, board, append=True)
        board += appended
        log = rl.leaves(batch, size, status_in=weeded, log=log).log
        root, store = rl.tree(log)
        if kept is None:
            n1 = len(log) // 32
            paths, _, _ = rl.paths([0, 77, n1 - 1], log, store)
            kept = (n1, root, paths)                                      # what a monitor and three voters hold after batch one
    n1, root1, paths1 = kept
    n2 = len(log) // 32
    leaves = [log[32 * i:32 * i + 32] for i in range(n2)]
    assert (n1, n2) == (150, 260) and root == M.mth(leaves) and root1 == M.mth(leaves[:n1]) != root
    heads, found = rl.heads([n1, n2], log, store)
    assert heads == [root1, root] and found == [0]                        # every head ever published, out of one rebuild
    proofs, _, lens = rl.consistency([n1], log, store)
    assert proofs[0] == b"".join(A.proof(n1, leaves)) and lens == [A.consistency_len(n1, n2)]
    assert rl.consistency_check([n1], [root1], proofs, n2, root) == ([0], [0, 0, 0, 0])
    # the receipts of batch one, as issued then, against the head kept then: proven, with no re-issue; against the new head they are not
    assert rl.check([0, 77, n1 - 1], b"".join(leaves[i] for i in (0, 77, n1 - 1)), paths1, n1, root1) == ([0, 0, 0], [0, 0, 0])
    assert all(rl.check([0, 77, n1 - 1], b"".join(leaves[i] for i in (0, 77, n1 - 1)), paths1, n2, root)[0])


def test_cpp_voting_example_with_heads(tmp_path):
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "voting.cpp"),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    out = subprocess.run([str(exe), "--receipts", "5", "--heads", "4", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "past heads: 4 of 4 consistency proofs proven against the head of 99 leaves" in out.stdout
    assert "forged old head: refused (old root mismatch)" in out.stdout and "OK: the decrypted totals equal the expected ones" in out.stdout
    plain = subprocess.run([str(exe), "--receipts", "5", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "past heads" not in plain.stdout                     # without the flag: byte for byte as before
    assert [line for line in out.stdout.splitlines() if "past heads" not in line] == plain.stdout.splitlines()
    alone = subprocess.run([str(exe), "--heads", "4", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert alone.returncode == 2 and "needs --receipts" in alone.stdout
