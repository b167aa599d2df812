"""The receipt log's grow entry (eg_merkle_grow / eg_merkle_grow_device) on the GPU: the node store and the root of N leaves out of the
node store of the first m.  Every expected value comes from the pure-Python model tests/merkle_ref.py (hashlib): store and root are
compared byte for byte, with canaries around every array the library writes, and the old store must come back unchanged.  What the
pass must never read is junk in every case: the old store's nodes (L, j) with (j + 1) 2^L > m and the leaves below (m >> 10) << 10,
while the expected values are the model's over the true leaves - a pass that rebuilds, or copies a ragged node, gives other bytes."""
import statistics
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
T = 10


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


class Buf:
    """device bytes `shift` bytes into an allocation, canaries in front and behind"""

    def __init__(self, torch, data=None, size=None, shift=0):
        self.size, self.shift = len(data) if data is not None else size, shift
        a = np.full(shift + self.size + PAD, CANARY, dtype=np.uint8)
        if data:
            a[shift:shift + self.size] = np.frombuffer(data, dtype=np.uint8)
        self.t = torch.from_numpy(a).cuda()
        self.ptr = self.t.data_ptr() + shift

    def bytes(self):
        return self.t.cpu().numpy().tobytes()[self.shift:self.shift + self.size]

    def intact(self):
        b = self.t.cpu().numpy().tobytes()
        return b[:self.shift] == bytes([CANARY]) * self.shift and b[self.shift + self.size:] == bytes([CANARY]) * PAD


def leaves_of(n, seed):
    raw = np.random.default_rng(seed).integers(0, 256, n * 32, dtype=np.uint8).tobytes()
    return [raw[32 * i:32 * i + 32] for i in range(n)]


LEAVES = leaves_of(5300, 22)            # every small case is a prefix of these
_models = {}


def model(n):
    """(root, levels) of the model over the first n of LEAVES, computed once per size and left unchanged"""
    if n not in _models:
        levels = M.levels(LEAVES[:n])
        _models[n] = (levels[-1][0] if n else M.mth([]), levels)
    return _models[n]


def store_of(levels):
    return b"".join(b"".join(lv) for lv in levels[1:])


def junk_old_store(levels, m):
    """the node store of m leaves with every node the grow must not read - (j + 1) 2^L > m - replaced by junk"""
    return b"".join(b"".join(lv[:m >> k]) + b"\xee" * 32 * (len(lv) - (m >> k)) for k, lv in enumerate(levels) if k)


def junk_log(leaves, m):
    first = (m >> T) << T
    return b"\xdd" * 32 * first + b"".join(leaves[first:])


def grow_dev(torch, eg, ctx, m, old_store, log, n, old_shift=0, new_shift=0, stream=0):
    """eg_merkle_grow_device on device arrays -> (root, store); canaries and the old store checked"""
    rl = eg.ReceiptLog(ctx)
    assert len(old_store) == rl.nodes_bytes(m) and len(log) == 32 * n
    d_old, d_log = Buf(torch, old_store, shift=old_shift), Buf(torch, log)
    d_new, d_root = Buf(torch, size=rl.nodes_bytes(n), shift=new_shift), Buf(torch, size=32)
    torch.cuda.synchronize()
    rl.grow_device(m, d_old.ptr, n, d_log.ptr, d_new.ptr, d_root.ptr, stream=stream)
    torch.cuda.synchronize()
    assert d_new.intact() and d_root.intact() and d_old.intact() and d_log.intact(), (m, n)
    assert d_old.bytes() == old_store and d_log.bytes() == log, (m, n)          # out of place: the inputs are as they were
    return d_root.bytes(), d_new.bytes()


def grow_case(torch, eg, ctx, m, n, old_shift=0, new_shift=0):
    root, levels = model(n)
    got = grow_dev(torch, eg, ctx, m, junk_old_store(model(m)[1], m), junk_log(LEAVES[:n], m), n, old_shift, new_shift)
    assert got[0] == root, (m, n)
    assert got[1] == store_of(levels), (m, n)


# ------------------------------------------------------------------ the seams of the tile
SEAM_M = (0, 1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049)
SEAM_D = (0, 1, 2, 1023, 1024, 1025)


def test_the_model_of_the_junk():
    """the helpers above against a direct statement of the contract"""
    for m in (0, 1, 5, 1024, 1025, 2049):
        levels = model(m)[1]
        junk, true = junk_old_store(levels, m), store_of(levels)
        assert len(junk) == len(true)
        off = 0
        for k in range(1, len(levels)):
            for j in range(len(levels[k])):
                keep = (j + 1) << k <= m
                assert junk[off:off + 32] == (levels[k][j] if keep else b"\xee" * 32), (m, k, j)
                off += 32
    assert junk_log(LEAVES[:1030], 1025) == b"\xdd" * 32768 + b"".join(LEAVES[1024:1030]) and junk_log(LEAVES[:9], 9) == b"".join(LEAVES[:9])
    assert model(0)[0] == M.H(b"") and model(1)[0] == LEAVES[0] and model(777)[0] == M.mth(LEAVES[:777])


@pytest.mark.parametrize("m", SEAM_M)
def test_seam_sweep(torch, eg, ctx, m):
    for d in SEAM_D:
        grow_case(torch, eg, ctx, m, m + d)


@pytest.mark.parametrize("m", SEAM_M)
def test_seam_sweep_with_both_stores_four_bytes_off(torch, eg, ctx, m):
    """the word path of the copy: neither store is 16-byte aligned"""
    for d in SEAM_D:
        grow_case(torch, eg, ctx, m, m + d, old_shift=4, new_shift=4)


def test_only_one_store_misaligned(torch, eg, ctx):
    grow_case(torch, eg, ctx, 2049, 2049 + 1025, old_shift=4, new_shift=0)
    grow_case(torch, eg, ctx, 2049, 2049 + 1025, old_shift=0, new_shift=12)
    grow_case(torch, eg, ctx, 2048, 2048, old_shift=8, new_shift=16)


# ------------------------------------------------------------------ the third launch and a depth change
BIG = ((1 << 20) - 1, (1 << 20) + 3, (1 << 20) + 1030)


def prefix_levels(levels, n):
    """the levels of the first n leaves out of the levels of more leaves, by the bottom-up rule of the model: level k keeps its first
    n >> k nodes, and the one node that may follow them is made from the level below"""
    out = [levels[0][:n]]
    for k in range(1, M.depth(n) + 1):
        a = out[-1]
        keep = n >> k
        out.append(levels[k][:keep] + [M.node_hash(a[2 * i], a[2 * i + 1]) if 2 * i + 1 < len(a) else a[2 * i] for i in range(keep, (len(a) + 1) // 2)])
    return out


@pytest.fixture(scope="module")
def big():
    """the model's levels of 2^20 + 1030 leaves, computed ONCE; the two smaller trees are prefixes of it"""
    leaves = leaves_of(BIG[2], 23)
    top = M.levels(leaves)
    for n in (0, 1, 2, 3, 5, 64, 65, 1023, 1025):                             # prefix_levels is the model's own rule
        assert prefix_levels(model(2100)[1], n) == model(n)[1], n
    return leaves, {BIG[2]: top, BIG[1]: prefix_levels(top, BIG[1]), BIG[0]: prefix_levels(top, BIG[0])}


@pytest.mark.parametrize("step", (0, 1))
def test_the_third_launch_and_a_depth_change(torch, eg, ctx, big, step):
    """2^20 - 1 -> 2^20 + 3: the depth grows from 20 to 21 and a third launch appears; 2^20 + 3 -> 2^20 + 1030: all three launches copy"""
    leaves, levels = big
    m, n = BIG[step], BIG[step + 1]
    assert (M.depth(BIG[0]), M.depth(BIG[1]), M.depth(BIG[2])) == (20, 21, 21)
    root, store = grow_dev(torch, eg, ctx, m, junk_old_store(levels[m], m), junk_log(leaves[:n], m), n)
    assert root == levels[n][-1][0] and len(levels[n]) == 22
    assert store == store_of(levels[n])


# ------------------------------------------------------------------ a chain of grows
def test_a_chain_of_five_grows_with_uneven_batches(torch, eg, ctx):
    """every store is grown out of the one the library grew before it, and equals the model's rebuild"""
    sizes = (0, 700, 1024, 1025, 3000, 5200)
    store = b""
    for m, n in zip(sizes, sizes[1:]):
        root, store = grow_dev(torch, eg, ctx, m, store, junk_log(LEAVES[:n], m), n)
        want_root, levels = model(n)
        assert root == want_root and store == store_of(levels), (m, n)


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def election(eg, ctx, oracle):
    pk = oracle.keypair_from_seed(12345)[1]
    return eg.ChoiceParams(ctx, pk, 5, True)


def test_end_to_end_two_batches_and_every_reader_on_the_grown_store(torch, eg, ctx, election):
    """two batches of generated ballots through verify -> weed -> leaves (append) -> grow; paths, heads, consistency and the two checks
    read the grown store as they read a rebuilt one"""
    p = election
    size = p.ballot_size
    fresh = p.encrypt_batch(2222, 0, 260)
    rl = eg.ReceiptLog(ctx, b"election-22")
    log, board, store, n_old, root1 = b"", b"", b"", 0, None
    for batch in (fresh[:150 * size], fresh[150 * size:]):
        n = len(batch) // size
        status, _ = p.verify_batch(batch)
        p.tally_reset()
        assert status == [0] * n
        dup, weeded, appended = p.weed(batch, status, board, append=True)
        board += appended
        log = rl.leaves(batch, size, status_in=weeded, log=log).log
        root, store = rl.grow(n_old, store, log)                          # batch one: out of the empty store, a full build
        n_old = len(log) // 32
        root1 = root1 or root
    n1, n2 = 150, n_old
    leaves = [log[32 * i:32 * i + 32] for i in range(n2)]
    assert n2 == 260 and root == M.mth(leaves) and store == M.node_store(leaves) and root1 == M.mth(leaves[:n1]) != root
    index = list(range(n2))
    paths, _, lens = rl.paths(index, log, store)
    assert paths == [b"".join(M.path(i, leaves)) for i in index]
    assert rl.check(index, log, paths, n2, root) == ([0] * n2, [0, 0, 0])     # every receipt is proven
    assert rl.heads([n1, n2, 0], log, store) == ([root1, root, M.H(b"")], [0])
    proofs, _, plens = rl.consistency([n1], log, store)
    assert proofs[0] == b"".join(A.proof(n1, leaves)) and plens == [A.consistency_len(n1, n2)]
    assert rl.consistency_check([n1], [root1], proofs, n2, root) == ([0], [0, 0, 0, 0])


# ------------------------------------------------------------------ the entry forms
def test_host_entry_against_the_device_entry_on_a_caller_stream(torch, eg, ctx):
    rl = eg.ReceiptLog(ctx)
    s = torch.cuda.Stream()
    for m, n in ((0, 0), (0, 1), (1, 1), (1, 2), (0, 1500), (700, 1500), (1024, 1500), (1500, 1500), (2048, 4096), (4096, 4096)):
        root, levels = model(n)
        old, log = junk_old_store(model(m)[1], m), junk_log(LEAVES[:n], m)
        on_stream = grow_dev(torch, eg, ctx, m, old, log, n, stream=s.cuda_stream)
        assert on_stream == (root, store_of(levels)), (m, n)
        assert rl.grow(m, old, log) == on_stream, (m, n)                 # the host form: the same bytes, and it sends no junk leaf either


def test_a_pass_beside_a_verifying_thread(torch, eg, ctx, election):
    """two threads grow stores on streams of their own while a third verifies ballots on the same context: the entry takes no lock and
    uses no workspace of the context"""
    p = election
    n_ballots = 1500
    d_msgs = torch.full((n_ballots * p.ballot_size + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(909, 0, n_ballots, d_msgs.data_ptr())
    p.ctx.synchronize()
    cases = ((1025, 3000), (2048, 5200))
    errors, results = [], {}

    def worker(k):
        try:
            s = torch.cuda.Stream()
            m, n = cases[k]
            old, log = junk_old_store(model(m)[1], m), junk_log(LEAVES[:n], m)
            results[k] = [grow_dev(torch, eg, ctx, m, old, log, n, stream=s.cuda_stream) for _ in range(3)]
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

    for m, n in cases:
        model(m), model(n)                                                 # the shared model is filled before the threads start
    threads = [threading.Thread(target=worker, args=(0,)), threading.Thread(target=worker, args=(1,)), threading.Thread(target=verifier)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    p.tally_reset()
    assert not errors, errors
    assert results["status"] == [0] * n_ballots
    for k, (m, n) in enumerate(cases):
        root, levels = model(n)
        assert results[k] == [(root, store_of(levels))] * 3


def test_refusals_with_a_live_context_launch_nothing(torch, eg, ctx):
    rl = eg.ReceiptLog(ctx)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    b = buf.data_ptr()
    old, log, new, root = b, b + 4096, b + 8192, b + 16384

    def refused(text, *args):
        with pytest.raises(eg.EgError, match=text):
            rl.grow_device(*args)

    refused("old_size is above N", 10, old, 9, log, new, root)
    refused("old_size is 2\\^31 or more", 1 << 31, old, 1 << 31, log, new, root)
    refused("N is 2\\^31 or more", 5, old, 1 << 31, log, new, root)
    refused("null root", 5, old, 9, log, new, 0)
    refused("null log", 5, old, 9, 0, new, root)
    refused("null nodes", 5, old, 9, log, 0, root)
    refused("null nodes_old", 5, 0, 9, log, new, root)
    refused("overlap", 5, old, 9, log, old + 188, root)
    refused("overlap", 5, new + 348, 9, log, new, root)
    for k in (1, 3, 4, 5):
        args = [5, old, 9, log, new, root]
        args[k] += 2
        refused("4-byte aligned", *args)
    torch.cuda.synchronize()
    assert int(buf.sum().item()) == 0                                          # nothing was launched


def test_cpp_voting_example_with_grow(tmp_path):
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "voting.cpp"),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    out = subprocess.run([str(exe), "--receipts", "5", "--heads", "4", "--grow", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "grown log: the tree of 99 leaves out of the tree of its first 49: root and node store equal the rebuild" in out.stdout
    assert "past heads: 4 of 4 consistency proofs proven against the head of 99 leaves" in out.stdout
    assert "OK: the decrypted totals equal the expected ones" in out.stdout
    plain = subprocess.run([str(exe), "--receipts", "5", "--heads", "4", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "grown log" not in plain.stdout                       # without the flag: byte for byte as before
    assert [line for line in out.stdout.splitlines() if "grown log" not in line] == plain.stdout.splitlines()
    alone = subprocess.run([str(exe), "--grow", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert alone.returncode == 2 and "needs --receipts" in alone.stdout


# ------------------------------------------------------------------ one guard, not a target
def test_a_grow_by_one_tile_takes_less_time_than_the_rebuild(torch, eg, ctx):
    """m = 2^22 -> N = 2^22 + 1024 on device-resident data, HIP events, the median of seven runs after two warm-ups, beside
    eg_merkle_tree_device (with its node store) of the same N in the same process.  The bound is a ratio below 1.0 and nothing tighter:
    it catches a grow that rebuilds.  The ratio is printed."""
    rl = eg.ReceiptLog(ctx)
    m, n = 1 << 22, (1 << 22) + 1024
    log = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, device="cuda")
    old, new, rebuilt = (torch.zeros(rl.nodes_bytes(k), dtype=torch.uint8, device="cuda") for k in (m, n, n))
    root, root2 = torch.zeros(32, dtype=torch.uint8, device="cuda"), torch.zeros(32, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rl.tree_device(m, log.data_ptr(), root.data_ptr(), old.data_ptr(), stream=stream)

    def median_ms(fn):
        ts = []
        for k in range(9):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if k >= 2:
                ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    tree_ms = median_ms(lambda: rl.tree_device(n, log.data_ptr(), root2.data_ptr(), rebuilt.data_ptr(), stream=stream))
    grow_ms = median_ms(lambda: rl.grow_device(m, old.data_ptr(), n, log.data_ptr(), new.data_ptr(), root.data_ptr(), stream=stream))
    torch.cuda.synchronize()
    assert torch.equal(new, rebuilt) and torch.equal(root, root2)            # the two stores it timed are the same bytes
    print(f"grow 2^22 -> 2^22 + 1024: {grow_ms:.3f} ms, rebuild {tree_ms:.3f} ms, ratio {grow_ms / tree_ms:.3f}")
    assert grow_ms / tree_ms < 1.0, (grow_ms, tree_ms)
