"""The receipt log (eg_merkle_* and their _device forms) on the GPU: leaf hashes of GPU-made ballots, trees at the seams of the tile
(T_LOG = 10: 1023 / 1024 / 1025, 2049, and 2^20 + 3 for the third launch), audit paths, and the check of many receipts.  Every expected
value comes from the pure-Python model tests/merkle_ref.py (hashlib, written from the RFC text); roots, node stores, paths, leaves and
the appended log are compared byte for byte, with canaries behind every array the library writes."""
import random
import statistics
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import merkle_ref as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CANARY = 0x5C
PAD = 64
TILE = 1 << 10
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
    """(raw log, leaves, root, node store) of the model, computed once per size and left unchanged"""
    if n not in _trees:
        raw, leaves = leaves_of(n, seed)
        levels = M.levels(leaves)
        root = levels[-1][0] if n else M.mth([])
        if n <= 4096:
            assert root == M.mth(leaves)                                  # the recursion of the RFC
        _trees[n] = (raw, leaves, root, b"".join(b"".join(lv) for lv in levels[1:]), levels)
    return _trees[n]


def tree_dev(torch, eg, ctx, raw, n, with_nodes=True, stream=0):
    rl = eg.ReceiptLog(ctx)
    d_log = dev(torch, raw)
    d_root = room(torch, 32)
    size = rl.nodes_bytes(n)
    d_nodes = room(torch, size) if with_nodes else None
    need = 0 if with_nodes else rl.tree_scratch_bytes(n)
    d_scratch = room(torch, need) if need else None
    torch.cuda.synchronize()
    rl.tree_device(n, d_log.data_ptr(), d_root.data_ptr(), d_nodes.data_ptr() if with_nodes else 0, d_scratch.data_ptr() if need else 0, need, stream)
    torch.cuda.synchronize()
    assert tail_ok(d_root, 32) and tail_ok(d_log, len(raw)) and (not with_nodes or tail_ok(d_nodes, size)) and (not need or tail_ok(d_scratch, need))
    return host(d_root, 32), (host(d_nodes, size) if with_nodes else None), d_log, d_nodes


# ------------------------------------------------------------------ trees
@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_tree_root_and_node_store_byte_for_byte(torch, eg, ctx, n):
    raw, leaves, root, store, _ = model_tree(n)
    got_root, got_store, _, _ = tree_dev(torch, eg, ctx, raw, n)
    assert got_root == root and got_store == store and len(store) == eg.ReceiptLog.nodes_bytes(n)
    bare_root, _, _, _ = tree_dev(torch, eg, ctx, raw, n, with_nodes=False)
    assert bare_root == root
    host_root, host_store = eg.ReceiptLog(ctx).tree(raw)
    assert host_root == root and host_store == store
    assert eg.ReceiptLog(ctx).tree(raw, with_nodes=False) == (root, None)


def test_tree_that_needs_the_third_launch(torch, eg, ctx):
    """2^20 + 3 leaves: two full launches of ten levels and a third for the top"""
    n = BIG
    assert eg.ReceiptLog.depth(n) == 21 > 2 * 10
    raw, leaves, root, store, levels = model_tree(n)
    got_root, got_store, d_log, d_nodes = tree_dev(torch, eg, ctx, raw, n)
    assert got_root == root
    assert got_store == store
    bare_root, _, _, _ = tree_dev(torch, eg, ctx, raw, n, with_nodes=False)
    assert bare_root == root
    # receipts at the seams of the tiles and of the tree
    index = [0, 63, 64, TILE - 1, TILE, TILE + 1, (1 << 20) - 1, 1 << 20, n - 1, n, n + 1]
    paths, lens, verdict, found = paths_and_check(torch, eg, ctx, index, n, d_log, d_nodes, leaves, root)
    for j, i in enumerate(index):
        if i >= n:
            assert lens[j] == M.NO_PATH and verdict[j] == M.BAD_INDEX and paths[j] == bytes(32 * 21)
        else:
            want = [levels[k][(i >> k) ^ 1] for k in range(21) if ((i >> k) ^ 1) < len(levels[k])]
            assert lens[j] == len(want) == M.path_len(i, n) and paths[j] == b"".join(want) + bytes(32 * (21 - len(want))), i
            assert verdict[j] == 0 == M.check(i, n, leaves[i], want, root), i
    assert found == [2, 0, 0]


# ------------------------------------------------------------------ paths and checks
def paths_and_check(torch, eg, ctx, index, n, d_log, d_nodes, leaves, root, stream=0):
    """paths_device for the indices, then check_device of (index, leaf, path, path_len) as issued -> (rows, path_len, verdicts, found)"""
    rl = eg.ReceiptLog(ctx)
    m, row = len(index), 32 * rl.depth(n)
    d_index = dev(torch, u64s(index))
    d_paths, d_len = room(torch, m * row), room(torch, 4 * m)
    ptr = lambda t: 0 if t is None else t.data_ptr()                      # noqa: E731
    torch.cuda.synchronize()
    rl.paths_device(m, d_index.data_ptr(), n, ptr(d_log), ptr(d_nodes), d_paths.data_ptr(), d_len.data_ptr(), stream)
    torch.cuda.synchronize()
    assert tail_ok(d_paths, m * row) and tail_ok(d_len, 4 * m)
    rows = host(d_paths, m * row)
    lens = np.frombuffer(host(d_len, 4 * m), dtype=np.uint32).tolist()
    d_leaves = dev(torch, b"".join(leaves[i] if i < n else bytes(32) for i in index))
    d_root = dev(torch, root)
    d_verdict, d_found = room(torch, 4 * m), dev(torch, u32s([77, 77, 77]))
    torch.cuda.synchronize()
    rl.check_device(m, d_index.data_ptr(), d_leaves.data_ptr(), d_paths.data_ptr(), row, d_len.data_ptr(), n, d_root.data_ptr(), d_verdict.data_ptr(),
                    d_found.data_ptr(), stream)
    torch.cuda.synchronize()
    assert tail_ok(d_verdict, 4 * m) and tail_ok(d_found, 12)
    verdict = np.frombuffer(host(d_verdict, 4 * m), dtype=np.uint32).tolist()
    found = np.frombuffer(host(d_found, 12), dtype=np.uint32).tolist()
    return [rows[j * row:(j + 1) * row] for j in range(m)], lens, verdict, found


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 8, 9, 63, 64, 65])
def test_paths_and_checks_of_every_leaf(torch, eg, ctx, n):
    raw, leaves, root, store, _ = model_tree(n)
    _, _, d_log, d_nodes = tree_dev(torch, eg, ctx, raw, n)
    index = list(range(n)) + [n, n + 1]
    rows, lens, verdict, found = paths_and_check(torch, eg, ctx, index, n, d_log, d_nodes, leaves, root)
    d = M.depth(n)
    for i in range(n):
        want = M.path(i, leaves)
        assert lens[i] == len(want) and rows[i] == b"".join(want) + bytes(32 * (d - len(want))), i
    assert lens[n:] == [M.NO_PATH] * 2 and rows[n:] == [bytes(32 * d)] * 2
    assert verdict == [0] * n + [M.BAD_INDEX] * 2 and found == [2, 0, 0]
    # the host forms say the same
    rl = eg.ReceiptLog(ctx)
    paths, raw_rows, host_lens = rl.paths(index, raw, store)
    assert raw_rows == b"".join(rows) and host_lens == lens and paths[n:] == [None, None]
    assert rl.check(index[:n], raw, paths[:n], n, root) == ([0] * n, [0, 0, 0])


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_paths_and_checks_at_the_tile_seams(torch, eg, ctx, n):
    raw, leaves, root, store, _ = model_tree(n)
    _, _, d_log, d_nodes = tree_dev(torch, eg, ctx, raw, n)
    index = sorted({0, 63, 64, 1022, 1023, 1024, 2047, 2048, n - 1} & set(range(n))) + [n, n + 1, 1 << 40]
    rows, lens, verdict, found = paths_and_check(torch, eg, ctx, index, n, d_log, d_nodes, leaves, root)
    d = M.depth(n)
    for j, i in enumerate(index[:-3]):
        want = M.path(i, leaves)
        assert lens[j] == len(want) and rows[j] == b"".join(want) + bytes(32 * (d - len(want))), i
    assert verdict == [0] * (len(index) - 3) + [M.BAD_INDEX] * 3 and found == [3, 0, 0]


def test_a_wavefront_of_forged_receipts_among_good_ones(torch, eg, ctx):
    """300 receipts of a 777-leaf tree: forgeries of every kind at lanes 0, 63, 64 and last and a whole wavefront (lanes 128 .. 191) of
    them; every verdict and the found words against the model.  The paths of receipts with a wrong length are never read: their rows lie
    with a stride that leaves room for the longer lengths."""
    n, m = 777, 300
    raw, leaves, root, store, _ = model_tree(n)
    rng = random.Random(9)
    rl = eg.ReceiptLog(ctx)
    d = M.depth(n)
    stride = 32 * (d + 2)
    index = [rng.randrange(n) for _ in range(m)]
    index[5], index[6] = n - 1, n - 2                                     # the short paths of the ragged edge
    recs = [[i, leaves[i], M.path(i, leaves)] for i in index]
    forged = {0: "leaf", 63: "path", 64: "index", m - 1: "short"}
    for lane in range(128, 192):
        forged[lane] = ("leaf", "path", "index", "short", "long", "other", "swap")[lane % 7]
    for lane, kind in forged.items():
        r = recs[lane]
        if kind == "leaf":
            r[1] = bytes([r[1][0] ^ 1]) + r[1][1:]
        elif kind == "path":
            k = lane % len(r[2])
            r[2] = r[2][:k] + [r[2][k][:31] + bytes([r[2][k][31] ^ 0x80])] + r[2][k + 1:]
        elif kind == "index":
            r[0] = n + lane
        elif kind == "short":
            r[2] = r[2][:-1]
        elif kind == "long":
            r[2] = r[2] + [bytes(32)]
        elif kind == "other":
            r[0] = (r[0] + 1) % n                                         # somebody else's index: same length or not, never proven
        elif kind == "swap":
            r[2] = [r[2][1], r[2][0]] + r[2][2:]
    want = [M.check(i, n, leaf, path, root) for i, leaf, path in recs]
    assert [want[k] for k in (0, 63, 64, m - 1)] == [M.MISMATCH, M.MISMATCH, M.BAD_INDEX, M.BAD_LENGTH]
    assert all(want[k] for k in forged) and sum(1 for w in want if w == 0) == m - len(forged) and {M.BAD_INDEX, M.BAD_LENGTH, M.MISMATCH} <= set(want[128:192])
    verdict, found = rl.check([r[0] for r in recs], b"".join(r[1] for r in recs), b"".join(b"".join(r[2]) + bytes(stride - 32 * len(r[2])) for r in recs), n, root,
                              path_len=[len(r[2]) for r in recs], path_stride=stride)
    assert verdict == want and found == [want.count(1), want.count(2), want.count(3)]
    # against the root of another tree nothing is proven
    other = model_tree(1025)[2]
    verdict, found = rl.check([r[0] for r in recs], b"".join(r[1] for r in recs), [b"".join(r[2]) for r in recs], n, other)
    assert all(verdict) and found[2] == sum(1 for w in want if w in (0, M.MISMATCH))


# ------------------------------------------------------------------ the leaf pass
@pytest.fixture(scope="module")
def elections(eg, ctx, oracle):
    pk = oracle.keypair_from_seed(12345)[1]
    return {"single": eg.ChoiceParams(ctx, pk, 5, True), "multi": eg.ChoiceParams(ctx, pk, 4, False), "qv": eg.QuadraticVotingParams(ctx, pk, 3, 10)}


def gpu_ballots(torch, p, n, seed):
    d = room(torch, n * p.ballot_size)
    if n and getattr(p, "single", True) is False:
        p.encrypt_batch_device(seed, 0, n, d.data_ptr(), 2)              # multi-choice: two options selected
    elif n:
        p.encrypt_batch_device(seed, 0, n, d.data_ptr())
    p.ctx.synchronize()
    return d, host(d, n * p.ballot_size)


def leaves_dev(torch, eg, ctx, d_msgs, n, size, prefix=b"", extra=None, status=None, n_prior=0, log=None, log_cap=0, want_out=True, stream=0):
    """the device entry with buffers of its own and a canary behind every array the library writes -> dict"""
    rl = eg.ReceiptLog(ctx, prefix)
    d_extra = None if extra is None else dev(torch, extra)
    d_status = None if status is None else dev(torch, u32s(status))
    d_index, d_out = room(torch, 8 * n), (room(torch, 32 * n) if want_out else None)
    append = log is not None
    d_log = dev(torch, log + bytes([0xA7]) * (32 * log_cap - len(log))) if append else None
    d_count = dev(torch, u64s([12345])) if append else None
    d_found = dev(torch, u32s([77, 77]))
    need = rl.leaves_scratch_bytes(n)
    d_scratch = room(torch, need)
    ptr = lambda t: 0 if t is None else t.data_ptr()                      # noqa: E731
    torch.cuda.synchronize()
    rl.leaves_device(n, ptr(d_msgs), size, size, d_index.data_ptr(), d_found.data_ptr(), d_scratch.data_ptr(), need, ptr(d_extra), 64 if extra else 0,
                     64 if extra else 0, ptr(d_status), n_prior, ptr(d_out), ptr(d_log), log_cap, ptr(d_count), stream)
    torch.cuda.synchronize()
    assert tail_ok(d_index, 8 * n) and tail_ok(d_found, 8) and tail_ok(d_scratch, need) and (d_out is None or tail_ok(d_out, 32 * n))
    res = {"leaf_index": np.frombuffer(host(d_index, 8 * n), dtype=np.uint64).tolist(), "leaves_out": host(d_out, 32 * n) if want_out else None,
           "found": np.frombuffer(host(d_found, 8), dtype=np.uint32).tolist()}
    if append:
        assert tail_ok(d_log, 32 * log_cap) and tail_ok(d_count, 8)
        res["log_count"] = int(np.frombuffer(host(d_count, 8), dtype=np.uint64)[0])
        res["log"] = host(d_log, 32 * log_cap)
    return res


def same_leaves(got, want, log=None, log_cap=0):
    assert got["leaf_index"] == want["leaf_index"] and got["found"] == want["found"]
    if got["leaves_out"] is not None:
        assert got["leaves_out"] == b"".join(want["leaves_out"])
    if log is not None:                                                   # byte for byte: the prior entries, the appended ones, nothing behind them
        assert got["log_count"] == want["log_count"]
        assert got["log"] == log + b"".join(want["appended"]) + bytes([0xA7]) * (32 * log_cap - len(log) - 32 * len(want["appended"]))


@pytest.mark.parametrize("kind", ["single", "multi", "qv"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_leaf_pass_against_hashlib(torch, eg, ctx, elections, kind, n):
    """GPU-made ballots (five-option single choice: 736 bytes; multi-choice and quadratic voting: other sizes and alignments), a prefix,
    the 64-byte signature slot as the extra, rejected ballots at lanes 0, 63, 64 and last whose bytes the model never sees"""
    p = elections[kind]
    size = p.ballot_size
    d_msgs, msgs = gpu_ballots(torch, p, n, 100 + n)
    extra = np.random.default_rng(n).integers(0, 256, 64 * n, dtype=np.uint8).tobytes()
    status = [0] * n
    for lane in (0, 63, 64, n - 1):
        if lane < n and n > 1:
            status[lane] = 6 | (lane << 8)
    items = [msgs[b * size:(b + 1) * size] for b in range(n)]
    extras = [extra[64 * b:64 * b + 64] for b in range(n)]
    prefix = b"election-19/" + kind.encode()
    prior = leaves_of(3, 1)[0]
    want = M.leaves_pass(items, prefix, extras, status, 3, 3 + n)
    got = leaves_dev(torch, eg, ctx, d_msgs, n, size, prefix, extra, status, 3, prior, 3 + n)
    same_leaves(got, want, prior, 3 + n)
    assert want["found"][0] == n - sum(1 for s in status if s)
    # status_in NULL, no extra, no prefix, no leaves_out, no append: every ballot has a leaf
    bare = leaves_dev(torch, eg, ctx, d_msgs, n, size, want_out=False, n_prior=1 << 30)
    assert bare["leaf_index"] == [(1 << 30) + b for b in range(n)] and bare["found"] == [n, 0]
    # the host form
    res = eg.ReceiptLog(ctx, prefix).leaves(msgs, size, extra=extra, extra_len=64, status_in=status, log=prior)
    assert res.leaf_index == want["leaf_index"] and res.leaves == b"".join(want["leaves_out"]) and res.log == prior + b"".join(want["appended"])
    assert res.found == want["found"]
    assert eg.ReceiptLog(ctx).leaves(msgs, size).leaves == b"".join(M.leaf_hash(m) for m in items)


_seam_batches = {}


def seam_batch(n):
    """(messages, status words, leaves, the model's pass with exact room, with one entry less) - computed once per size, left unchanged"""
    if n not in _seam_batches:
        msgs = np.random.default_rng(n).integers(0, 256, 8 * n, dtype=np.uint8).tobytes()
        status = [0] * n
        for lane in (0, 1023, 1024, 65535, 65536, n - 1):
            if lane < n:
                status[lane] = 6 | (lane << 8)
        items = [msgs[8 * b:8 * b + 8] for b in range(n)]
        kept = status.count(0)
        _seam_batches[n] = (msgs, status, kept, M.leaves_pass(items, b"", None, status, 0, kept), M.leaves_pass(items, b"", None, status, 0, kept - 1))
    return _seam_batches[n]


@pytest.mark.parametrize("n", [TILE + 1, 65 * TILE + 1])
def test_leaf_pass_at_the_seams_of_the_scan(torch, eg, ctx, n):
    """the ranks across a tile of the scan (1024 ballots) and across the second round of its tile sums (64 tiles): 8-byte messages, rejected
    ballots on both sides of every seam and at the end; a log with room for exactly the leaves takes them all, one entry less takes none"""
    msgs, status, kept, want_fit, want_short = seam_batch(n)
    d_msgs = dev(torch, msgs)
    got = leaves_dev(torch, eg, ctx, d_msgs, n, 8, status=status, log=b"", log_cap=kept)
    same_leaves(got, want_fit, b"", kept)
    last = max(b for b in range(n) if status[b] == 0)
    assert got["found"] == [kept, 0] and got["log_count"] == kept and got["leaf_index"][last] == kept - 1
    got = leaves_dev(torch, eg, ctx, d_msgs, n, 8, status=status, log=b"", log_cap=kept - 1)
    same_leaves(got, want_short, b"", kept - 1)
    assert got["found"] == [kept, 1] and got["log_count"] == 0 and got["log"] == bytes([0xA7]) * (32 * (kept - 1))
    assert tail_ok(d_msgs, 8 * n)


def test_two_batches_through_one_log_and_the_append_that_does_not_fit(torch, eg, ctx, elections):
    p = elections["single"]
    size = p.ballot_size
    d_a, a = gpu_ballots(torch, p, 100, 31)
    d_b, b = gpu_ballots(torch, p, 70, 32)
    st_a, st_b = [0 if k % 9 else 4 for k in range(100)], [0 if k % 5 else 2 for k in range(70)]
    items_a, items_b = [a[k * size:(k + 1) * size] for k in range(100)], [b[k * size:(k + 1) * size] for k in range(70)]
    cap = 150
    want_a = M.leaves_pass(items_a, b"id", None, st_a, 0, cap)
    got_a = leaves_dev(torch, eg, ctx, d_a, 100, size, b"id", None, st_a, 0, b"", cap)
    same_leaves(got_a, want_a, b"", cap)
    log = b"".join(want_a["appended"])
    n_a = want_a["log_count"]
    want_b = M.leaves_pass(items_b, b"id", None, st_b, n_a, cap)
    got_b = leaves_dev(torch, eg, ctx, d_b, 70, size, b"id", None, st_b, n_a, log, cap)
    same_leaves(got_b, want_b, log, cap)
    assert want_b["leaf_index"][1] == n_a and want_b["log_count"] == n_a + 56 and want_b["found"] == [56, 0]
    # the exact fit, and one entry short: nothing is appended, the count stays, found[1] is set, the other outputs are written
    for cap2, fits in ((n_a + 56, True), (n_a + 55, False), (n_a, False)):
        want = M.leaves_pass(items_b, b"id", None, st_b, n_a, cap2)
        got = leaves_dev(torch, eg, ctx, d_b, 70, size, b"id", None, st_b, n_a, log, cap2)
        same_leaves(got, want, log, cap2)
        assert got["found"] == [56, 0 if fits else 1] and got["log_count"] == (cap2 if fits else n_a)
    lib = eg._load()
    import ctypes as C
    index, out, count, found = (C.c_uint64 * 70)(), C.create_string_buffer(32 * 70), C.c_uint64(9), (C.c_uint32 * 2)()
    buf = C.create_string_buffer(log + bytes([0xA7]) * (32 * 55), 32 * (n_a + 55))
    rc = lib.eg_merkle_leaves(ctx._h, 70, b, size, size, b"id", 2, None, 0, 0, (C.c_uint32 * 70)(*st_b), n_a, index, out, buf, n_a + 55, C.byref(count), found)
    assert rc == -3 and b"do not fit" in lib.eg_last_error()              # EG_ERR_BAD_ARG after the outputs were written
    assert list(index) == want_b["leaf_index"] and out.raw == b"".join(want_b["leaves_out"]) and count.value == n_a and list(found) == [56, 1]
    assert buf.raw == log + bytes([0xA7]) * (32 * 55)


def test_entry_forms_agree_on_a_caller_stream(torch, eg, ctx, elections):
    p = elections["single"]
    size, n = p.ballot_size, 300
    d_msgs, msgs = gpu_ballots(torch, p, n, 77)
    status = [0 if k % 4 else 3 for k in range(n)]
    s = torch.cuda.Stream()
    got = leaves_dev(torch, eg, ctx, d_msgs, n, size, b"x", None, status, 0, b"", n, stream=s.cuda_stream)
    rl = eg.ReceiptLog(ctx, b"x")
    res = rl.leaves(msgs, size, status_in=status, log=b"")
    assert res.leaf_index == got["leaf_index"] and res.leaves == got["leaves_out"] and res.log == got["log"][:32 * got["log_count"]] and res.found == got["found"]
    log = res.log
    count = len(log) // 32
    root, store = rl.tree(log)
    got_root, got_store, d_log, d_nodes = tree_dev(torch, eg, ctx, log, count, stream=s.cuda_stream)
    assert (got_root, got_store) == (root, store)
    leaves = [log[32 * i:32 * i + 32] for i in range(count)]
    assert root == M.mth(leaves)
    index = list(range(0, count, 7)) + [count]
    rows, lens, verdict, found = paths_and_check(torch, eg, ctx, index, count, d_log, d_nodes, leaves, root, stream=s.cuda_stream)
    paths, raw_rows, host_lens = rl.paths(index, log, store)
    assert raw_rows == b"".join(rows) and host_lens == lens
    assert rl.check(index, b"".join(leaves[i] if i < count else bytes(32) for i in index), raw_rows, count, root, path_len=[0 if x == M.NO_PATH else x for x in lens],
                    path_stride=32 * M.depth(count)) == (verdict, found)
    assert verdict == [0] * (len(index) - 1) + [M.BAD_INDEX]


def test_n_zero(torch, eg, ctx):
    rl = eg.ReceiptLog(ctx, b"p")
    got = leaves_dev(torch, eg, ctx, None, 0, 736, b"p", None, None, 5, leaves_of(5, 2)[0], 9)
    assert got["leaf_index"] == [] and got["found"] == [0, 0] and got["log_count"] == 5 and got["log"] == leaves_of(5, 2)[0] + bytes([0xA7]) * 128
    res = rl.leaves(b"", 736, log=b"", n=0)
    assert res.leaf_index == [] and res.leaves == b"" and res.log == b"" and res.found == [0, 0]
    assert rl.tree(b"") == (M.H(b""), b"")
    assert rl.paths([], b"", b"") == ([], b"", []) and rl.check([], b"", [], 0, M.H(b"")) == ([], [0, 0, 0])
    d_found = dev(torch, u32s([7, 7, 7]))
    rl.check_device(0, 0, 0, 0, 96, 0, 5, 0, 0, d_found.data_ptr())
    rl.paths_device(0, 0, 5, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert host(d_found, 12) == u32s([0, 0, 0]) and tail_ok(d_found, 12)


def test_every_refusal_with_a_live_context(torch, eg, ctx):
    rl = eg.ReceiptLog(ctx)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    b = buf.data_ptr()
    big = 1 << 31

    def refused(text, fn, *args, **kw):
        with pytest.raises(eg.EgError, match=text):
            fn(*args, **kw)

    need = rl.leaves_scratch_bytes(4)
    refused("n is 2\\^31 or more", rl.leaves_device, big, b, 40, 40, b, b, b, 1 << 40)
    refused("msg_stride is below msg_len", rl.leaves_device, 4, b, 39, 40, b, b, b, need)
    refused("extra_stride is below extra_len", rl.leaves_device, 4, b, 40, 40, b, b, b, need, d_extra=b, extra_stride=63, extra_len=64)
    refused("null extra with a length", rl.leaves_device, 4, b, 40, 40, b, b, b, need, extra_stride=64, extra_len=64)
    refused("null msgs", rl.leaves_device, 4, 0, 40, 40, b, b, b, need)
    refused("null leaf_index or found", rl.leaves_device, 4, b, 40, 40, 0, b, b, need)
    refused("null leaf_index or found", rl.leaves_device, 4, b, 40, 40, b, 0, b, need)
    refused("n_prior is 2\\^31 or more", rl.leaves_device, 4, b, 40, 40, b, b, b, need, n_prior=big)
    refused("n_prior is above log_cap", rl.leaves_device, 4, b, 40, 40, b, b, b, need, n_prior=6, d_log=b, log_cap=5, d_log_count=b)
    refused("null log with an append", rl.leaves_device, 4, b, 40, 40, b, b, b, need, log_cap=5, d_log_count=b)
    refused("scratch is null or too small", rl.leaves_device, 4, b, 40, 40, b, b, 0, need)
    refused("scratch is null or too small", rl.leaves_device, 4, b, 40, 40, b, b, b, need - 1)
    refused("8-byte aligned", rl.leaves_device, 4, b, 40, 40, b + 4, b, b, need)
    refused("8-byte aligned", rl.leaves_device, 4, b, 40, 40, b, b, b, need, d_log=b, log_cap=9, d_log_count=b + 4)
    for kw in ({"d_leaves_out": b + 2}, {"d_status_in": b + 1}, {"d_log": b + 2, "log_cap": 9, "d_log_count": b}):
        refused("4-byte aligned", rl.leaves_device, 4, b, 40, 40, b, b, b, need, **kw)
    refused("4-byte aligned", rl.leaves_device, 4, b, 40, 40, b, b + 2, b, need)
    long_prefix = eg.ReceiptLog(ctx, bytes(256))
    refused("prefix_len is above 255", long_prefix.leaves_device, 4, b, 40, 40, b, b, b, need)
    refused("N is 2\\^31 or more", rl.tree_device, big, b, b, b)
    refused("null root", rl.tree_device, 5, b, 0, b)
    refused("null log", rl.tree_device, 5, 0, b, b)
    refused("scratch is null or too small", rl.tree_device, 1025, b, b, 0, 0, 0)
    refused("scratch is null or too small", rl.tree_device, 1025, b, b, 0, b, rl.tree_scratch_bytes(1025) - 1)
    for args in ((5, b + 2, b, b), (5, b, b + 1, b), (5, b, b, b + 2)):
        refused("4-byte aligned", rl.tree_device, *args)
    refused("m is 2\\^31 or more", rl.paths_device, big, b, 5, b, b, b, b)
    refused("N is 2\\^31 or more", rl.paths_device, 1, b, big, b, b, b, b)
    refused("null index or path_len", rl.paths_device, 1, 0, 5, b, b, b, b)
    refused("null index or path_len", rl.paths_device, 1, b, 5, b, b, b, 0)
    for args in ((1, b, 5, 0, b, b, b), (1, b, 5, b, 0, b, b), (1, b, 5, b, b, 0, b)):
        refused("null log, nodes or paths", rl.paths_device, *args)
    refused("8-byte aligned", rl.paths_device, 1, b + 4, 5, b, b, b, b)
    refused("4-byte aligned", rl.paths_device, 1, b, 5, b, b, b + 2, b)
    refused("m is 2\\^31 or more", rl.check_device, big, b, b, b, 96, b, 5, b, b, b)
    refused("N is 2\\^31 or more", rl.check_device, 1, b, b, b, 992, b, big, b, b, b)
    refused("path_stride is below 32 \\* depth", rl.check_device, 1, b, b, b, 95, b, 5, b, b, b)
    refused("path_stride is below 32 \\* depth", rl.check_device, 1, b, b, b, 64, b, 5, b, b, b)
    refused("path_stride is no multiple of 4", rl.check_device, 1, b, b, b, 98, b, 5, b, b, b)
    refused("null paths", rl.check_device, 1, b, b, 0, 96, b, 5, b, b, b)
    for k in (1, 2, 5, 7, 8, 9):
        args = [1, b, b, b, 96, b, 5, b, b, b]
        args[k] = 0
        refused("null index, leaves, path_len, root, verdict or found", rl.check_device, *args)
    refused("8-byte aligned", rl.check_device, 1, b + 4, b, b, 96, b, 5, b, b, b)
    for k in (2, 3, 5, 7, 8, 9):
        args = [1, b, b, b, 96, b, 5, b, b, b]
        args[k] = b + 2
        refused("4-byte aligned", rl.check_device, *args)
    torch.cuda.synchronize()
    assert int(buf.sum().item()) == 0                                          # nothing was launched


def test_a_pass_beside_a_verifying_thread(torch, eg, ctx, elections):
    """two threads hash leaves, build trees and check receipts on streams of their own while a third verifies ballots on the same
    context: the entries take no lock and use no workspace of the context"""
    p = elections["single"]
    size, n = p.ballot_size, 1500
    d_msgs, msgs = gpu_ballots(torch, p, n, 808)
    items = [msgs[b * size:(b + 1) * size] for b in range(n)]
    status = [0 if b % 11 else 7 for b in range(n)]
    want = M.leaves_pass(items, b"t", None, status, 0, n)
    log = b"".join(want["appended"])
    count = want["log_count"]
    root = M.mth(want["appended"])
    errors, results = [], {}

    def worker(k):
        try:
            s = torch.cuda.Stream()
            runs = []
            for _ in range(3):
                got = leaves_dev(torch, eg, ctx, d_msgs, n, size, b"t", None, status, 0, b"", n, stream=s.cuda_stream)
                got_root, _, d_log, d_nodes = tree_dev(torch, eg, ctx, got["log"][:32 * got["log_count"]], got["log_count"], stream=s.cuda_stream)
                runs.append((got, got_root, paths_and_check(torch, eg, ctx, [0, 1, count - 1, count], count, d_log, d_nodes, want["appended"], got_root, s.cuda_stream)))
            results[k] = runs
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    def verifier():
        try:
            s = torch.cuda.Stream()
            st = torch.full((n,), 9, dtype=torch.int32, device="cuda")
            for _ in range(3):
                p.verify_batch_device(n, d_msgs.data_ptr(), st.data_ptr(), stream=s.cuda_stream)
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
    assert results["status"] == [0] * n
    for k in (0, 1):
        for got, got_root, (_, lens, verdict, found) in results[k]:
            same_leaves(got, want, b"", n)
            assert got_root == root and verdict == [0, 0, 0, M.BAD_INDEX] and found == [1, 0, 0] and lens[3] == M.NO_PATH


# ------------------------------------------------------------------ end to end
def test_end_to_end_verify_weed_leaves_tree_receipts(torch, eg, ctx, elections):
    """300 generated ballots and 20 byte-for-byte copies in two batches: verify -> weed -> leaves over weeding's status_out -> tree.  The
    receipts of all 300 prove against the root, no flagged copy has a leaf, and a receipt issued from the first batch's tree fails against
    the two-batch root and proves once it is re-issued."""
    p = elections["single"]
    size = p.ballot_size
    fresh = p.encrypt_batch(4040, 0, 300)
    copies = [(17 * k + 3) % 150 for k in range(20)]
    first = fresh[:150 * size] + b"".join(fresh[c * size:(c + 1) * size] for c in copies[:10])
    second = fresh[150 * size:] + b"".join(fresh[c * size:(c + 1) * size] for c in copies[10:])
    rl = eg.ReceiptLog(ctx, b"election-19")
    log, board, receipts, trees = b"", b"", {}, []
    for batch in (first, second):
        n = len(batch) // size
        status, _ = p.verify_batch(batch)
        p.tally_reset()
        assert status == [0] * n                                          # a copy verifies: the proofs bind nothing of the voter
        dup, weeded, appended = p.weed(batch, status, board, append=True)
        board += appended
        n_prior = len(log) // 32
        res = rl.leaves(batch, size, status_in=weeded, log=log)
        log = res.log
        flagged = [b for b in range(n) if weeded[b]]
        assert flagged == list(range(150, n)) and all(res.leaf_index[b] == M.LEAF_NONE for b in flagged)          # no flagged copy has a leaf
        assert [res.leaf_index[b] for b in range(150)] == list(range(n_prior, n_prior + 150)) and res.found == [150, 0]
        items = [batch[b * size:(b + 1) * size] for b in range(150)]
        assert log[32 * n_prior:] == b"".join(M.leaf_hash(m, b"election-19") for m in items)
        root, store = rl.tree(log)
        count = len(log) // 32
        paths, _, lens = rl.paths(list(range(n_prior, count)), log, store)
        trees.append((count, root))
        for k, i in enumerate(range(n_prior, count)):
            receipts[i] = (log[32 * i:32 * i + 32], paths[k])
    (n1, root1), (n2, root2) = trees
    assert (n1, n2) == (150, 300) and root2 == M.mth([log[32 * i:32 * i + 32] for i in range(300)]) and root1 != root2
    every = list(range(300))
    reissued, _, _ = rl.paths(every, log, rl.tree(log)[1])
    verdict, found = rl.check(every, log, reissued, 300, root2)
    assert verdict == [0] * 300 and found == [0, 0, 0]                    # the receipts of all 300 prove against the root
    assert reissued[150:] == [receipts[i][1] for i in range(150, 300)]
    # a receipt from the first batch's tree: proven against its own root, not against the two-batch root (its path is one entry short
    # of the new tree's: judged by the length; with the new length's worth of bytes: by the root), proven once re-issued
    old = [receipts[i][1] for i in range(150)]
    assert rl.check(every[:150], log[:32 * 150], old, 150, root1) == ([0] * 150, [0, 0, 0])
    verdict, found = rl.check(every[:150], log[:32 * 150], old, 300, root2)
    assert all(v in (M.BAD_LENGTH, M.MISMATCH) for v in verdict) and found[0] == 0 and found[1] + found[2] == 150
    assert verdict == [M.check(i, 300, log[32 * i:32 * i + 32], [old[i][32 * k:32 * k + 32] for k in range(len(old[i]) // 32)], root2) for i in range(150)]
    assert rl.check(every[:150], log[:32 * 150], reissued[:150], 300, root2) == ([0] * 150, [0, 0, 0])


def test_cpp_voting_example_with_receipts(tmp_path):
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "voting.cpp"),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    out = subprocess.run([str(exe), "--receipts", "5", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "99 of 100 ballots verified" in out.stdout and "receipt log: 99 leaves, root " in out.stdout
    assert out.stdout.count(" path entries, proven") == 5 and "receipt of voter #5: leaf 3, " in out.stdout          # voter #4 is rejected
    assert "forged receipt: refused (root mismatch)" in out.stdout and "OK: the decrypted totals equal the expected ones" in out.stdout
    plain = subprocess.run([str(exe), "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "receipt" not in plain.stdout                        # the existing flags behave as before
    assert [line for line in out.stdout.splitlines() if "receipt" not in line] == plain.stdout.splitlines()
    qv = subprocess.run([str(exe), "--qv", "--receipts", "2", "40", "3", "10", "7"], capture_output=True, text=True, timeout=120)
    assert qv.returncode == 0 and qv.stdout.count(" path entries, proven") == 2 and "forged receipt: refused" in qv.stdout, qv.stdout + qv.stderr


# ------------------------------------------------------------------ a loose guard against a path that fell off the GPU
def test_leaf_pass_and_tree_are_cheaper_than_verifying_the_ballots(torch, eg, ctx, elections):
    """2^16 five-option ballots: the leaf pass plus the tree, call plus synchronize, take less time than the verify call for the same
    ballots in the same process (warm, median of three).  No margin: the expected ratio is below a tenth (profiles/r19_receipt_log.txt)."""
    import time

    p = elections["single"]
    size, n = p.ballot_size, 1 << 16
    d_msgs = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(5150, 0, n, d_msgs.data_ptr())
    rl = eg.ReceiptLog(ctx, b"election-19")
    st = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    d_index, d_log = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    d_count, d_found = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    need = rl.leaves_scratch_bytes(n)
    d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    d_root, d_nodes = torch.zeros(32, dtype=torch.uint8, device="cuda"), torch.zeros(rl.nodes_bytes(n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        ms = []
        for _ in range(4):                       # the first round warms up
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms[1:])

    verify_ms = timed(lambda: p.verify_batch_device(n, d_msgs.data_ptr(), st.data_ptr(), stream=stream))
    p.tally_reset()

    def receipts():
        rl.leaves_device(n, d_msgs.data_ptr(), size, size, d_index.data_ptr(), d_found.data_ptr(), d_scratch.data_ptr(), need, d_status_in=st.data_ptr(),
                         d_log=d_log.data_ptr(), log_cap=n, d_log_count=d_count.data_ptr(), stream=stream)
        rl.tree_device(n, d_log.data_ptr(), d_root.data_ptr(), d_nodes.data_ptr(), stream=stream)

    log_ms = timed(receipts)
    print(f"n = 2^16 five-option ballots: leaf pass + tree {log_ms:.3f} ms, verify {verify_ms:.3f} ms, ratio {log_ms / verify_ms:.4f}")
    assert int(st.abs().sum().item()) == 0 and int(d_count.item()) == n and d_found.cpu().tolist() == [n, 0]
    # the tree is the model's: the root over the log that the pass appended
    log = host(d_log)
    assert host(d_root) == M.levels([log[32 * i:32 * i + 32] for i in range(n)])[-1][0]
    assert log_ms < verify_ms
