"""Voter signatures on the GPU (eg_ed25519_*, eg_sha512_*).  Every expected value comes from hashlib, from the OpenSSL-made fixture
tests/golden/ed25519_openssl.json or from the RFC 8032 model in tests/ed25519_ref.py; every comparison is on bytes and status words."""
import hashlib
import json
import statistics
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import ed25519_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = [{k: bytes.fromhex(v) if k != "source" else v for k, v in e.items()}
           for e in json.loads((ROOT / "tests" / "golden" / "ed25519_openssl.json").read_text())["entries"]]
BAD = lambda detail: R.status_word(detail)          # noqa: E731
CANARY = 0x5C


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


@pytest.fixture(scope="module")
def ed(eg, ctx):
    return eg.Ed25519(ctx)


def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def flip(b: bytes, bit: int) -> bytes:
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def dev(torch, data: bytes):
    return torch.frombuffer(bytearray(data or b"\0"), dtype=torch.uint8).cuda()


def u32(torch, values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def as_u32(t):
    return [v & 0xFFFFFFFF for v in t.cpu().tolist()]


def verify_dev(torch, ed, msgs, msg_len, keys, sigs, prefix=b"", key_index=None, status_in=None, alias=False, stride=None, stream=0):
    """the device entry with buffers of its own and a canary behind the scratch and behind status_out -> status words"""
    n = len(sigs) // 64
    stride = msg_len if stride is None else stride
    need = ed.verify_scratch_bytes(n)
    scratch = torch.full((need + 64,), CANARY, dtype=torch.uint8, device="cuda")
    d_msgs, d_keys, d_sigs = dev(torch, msgs), dev(torch, keys), dev(torch, sigs)
    d_idx = None if key_index is None else u32(torch, key_index)
    d_in = None if status_in is None else u32(torch, list(status_in) + [0x5C5C5C5C] * 16 if alias else status_in)
    out = d_in if alias else torch.full((n + 16,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ed.verify_device(n, d_msgs.data_ptr(), stride, msg_len, d_keys.data_ptr(), len(keys) // 32, d_sigs.data_ptr(), out.data_ptr(), scratch.data_ptr(), need,
                     prefix=prefix, d_key_index=0 if d_idx is None else d_idx.data_ptr(), d_status_in=0 if d_in is None else d_in.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert bytes(scratch[need:].cpu().numpy()) == bytes([CANARY]) * 64, "the pass wrote behind its scratch"
    assert as_u32(out[n:]) == [0x5C5C5C5C] * 16, "the pass wrote behind status_out"
    return as_u32(out[:n])


def signed_items(ed, n, msg_len, prefix=b"", seed=1):
    """n GPU-signed items: (seeds, keys, msgs, sigs)"""
    seeds, msgs = rand(seed, 32 * n), rand(seed + 1000, msg_len * n)
    return seeds, ed.keypairs(seeds), msgs, ed.sign(seeds, msgs, msg_len, prefix)


def item(b: bytes, i: int, size: int) -> bytes:
    return b[i * size:(i + 1) * size]


# ------------------------------------------------------------------ the fixture
def test_fixture_entries_are_accepted_and_their_twins_rejected_with_the_models_words(ed):
    for e in FIXTURE:
        pk, m, s = e["public_key"], e["message"], e["signature"]
        twins = [(pk, m, s), (pk, m, flip(s, 7)), (pk, m, flip(s, 256 + 3)), (flip(pk, 11), m, s)]
        if m:
            twins.append((pk, flip(m, 8 * len(m) - 1), s))
        got = ed.verify(b"".join(t[1] for t in twins), len(m), b"".join(t[0] for t in twins), b"".join(t[2] for t in twins))
        want = [R.status_word(R.verify_detail(*t)) for t in twins]
        assert got == want and want[0] == 0 and all(want[1:]), (len(m), got, want)


def test_signer_and_key_pairs_reproduce_the_fixture_bytes(ed):
    assert ed.keypairs(b"".join(e["seed"] for e in FIXTURE)) == b"".join(e["public_key"] for e in FIXTURE)
    for e in FIXTURE:
        assert ed.sign(e["seed"], e["message"], len(e["message"])) == e["signature"], len(e["message"])


# ------------------------------------------------------------------ SHA-512
def test_sha512_of_every_length_with_a_poisoned_gap(ed):
    for msg_len in range(0, 301):
        stride, n = msg_len + 5, 3
        buf = bytearray(rand(msg_len, stride * n))
        msgs = [bytes(buf[b * stride:b * stride + msg_len]) for b in range(n)]
        for b in range(n):
            buf[b * stride + msg_len:(b + 1) * stride] = b"\xEE" * 5            # never hashed
        got = ed.sha512(bytes(buf)[: (n - 1) * stride + msg_len], msg_len, stride=stride, n=n)
        assert got == b"".join(hashlib.sha512(m).digest() for m in msgs), msg_len


def test_sha512_prefix_lengths_around_the_block_seams(ed):
    for plen in (0, 1, 63, 64, 255):
        prefix = rand(plen + 7, plen)
        for total in (111, 112, 113, 127, 128, 129, 255, 256, 257):
            if total < plen:
                continue
            msg_len = total - plen
            msgs = rand(total, 2 * msg_len)
            got = ed.sha512(msgs, msg_len, prefix=prefix, n=2)
            assert got == b"".join(hashlib.sha512(prefix + item(msgs, b, msg_len)).digest() for b in range(2)), (plen, total)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sha512_batches(ed, n):
    msgs = rand(n, 100 * n)
    assert ed.sha512(msgs, 100, prefix=b"election-7") == b"".join(hashlib.sha512(b"election-7" + item(msgs, b, 100)).digest() for b in range(n))


# ------------------------------------------------------------------ verify: sizes and lanes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_tampered_items_at_the_seams_of_wavefronts_and_blocks(torch, ed, n):
    prefix, msg_len = b"election/2026/7", 40
    seeds, keys, msgs, sigs = signed_items(ed, n, msg_len, prefix, seed=n)
    tampered = {i for i in (0, 63, 64, n - 1) if i < n}
    if n == 257:
        tampered |= set(range(128, 192))                       # a whole wavefront
    s = bytearray(sigs)
    for k, i in enumerate(sorted(tampered)):
        s[64 * i + (k % 64)] ^= 1 << (k % 8)                   # R or S of item i
    s = bytes(s)
    got = verify_dev(torch, ed, msgs, msg_len, keys, s, prefix)
    want = [R.expected_status(item(keys, i, 32), prefix + item(msgs, i, msg_len), item(s, i, 64), i in tampered) if i in tampered or i < 70 else 0
            for i in range(n)]
    assert got == want
    assert all(want[i] for i in tampered) and sum(1 for w in want if w) == len(tampered)
    assert ed.verify(msgs, msg_len, keys, s, prefix) == want               # the host entry


def test_every_kind_of_tampering(torch, ed):
    prefix, msg_len, n = b"\x00election\xff", 57, 12
    seeds, keys, msgs, sigs = signed_items(ed, n, msg_len, prefix, seed=77)
    roster = keys + R.small_order_encodings()[1] + R.small_order_encodings()[0]          # entries 12 (order 8) and 13 (the identity)
    idx = list(range(n))
    K, M, S = [item(keys, i, 32) for i in range(n)], [item(msgs, i, msg_len) for i in range(n)], [item(sigs, i, 64) for i in range(n)]
    S[1] = flip(S[1], 5)                                                   # a bit in R
    S[2] = flip(S[2], 256 + 100)                                           # a bit in S
    M[3] = flip(M[3], 0)                                                   # a bit in the message
    S[4] = S[4][:32] + (int.from_bytes(S[4][32:], "little") + R.L).to_bytes(32, "little")      # S + l: the same residue, not canonical
    idx[5] = 12                                                            # a small-order key
    idx[6] = 14                                                            # an index out of range
    idx[7] = 8                                                             # a right signature under a wrong roster index
    idx[8] = 13                                                            # the identity as key
    S[9] = flip(S[9], 255)                                                 # the sign bit of R
    S[10] = flip(S[10], 511)                                               # the top bit of S: far above l
    want = []
    for i in range(n):
        want.append(BAD(R.BAD_INDEX) if idx[i] >= 14 else R.status_word(R.verify_detail(item(roster, idx[i], 32), prefix + M[i], S[i])))
    assert want == [0, BAD(4), BAD(4), BAD(4), BAD(1), BAD(3), BAD(5), BAD(4), BAD(3), BAD(4), BAD(1), 0]
    got = verify_dev(torch, ed, b"".join(M), msg_len, roster, b"".join(S), prefix, key_index=idx)
    assert got == want
    # a bit in A (per-item keys, so only that item's key changes): the model decides between "does not decode" and "mismatch"
    K2 = list(K)
    for i, bit in enumerate((0, 1, 100, 254, 255, 77)):
        K2[i] = flip(K[i], bit)
    want2 = [R.status_word(R.verify_detail(K2[i], prefix + item(msgs, i, msg_len), item(sigs, i, 64))) for i in range(n)]
    assert all(want2[:6]) and not any(want2[6:]) and set(want2[:6]) <= {BAD(2), BAD(4)}
    assert verify_dev(torch, ed, msgs, msg_len, b"".join(K2), sigs, prefix) == want2
    # a bit in the prefix: nothing verifies
    assert verify_dev(torch, ed, msgs, msg_len, keys, sigs, flip(prefix, 3)) == [BAD(4)] * n
    assert verify_dev(torch, ed, msgs, msg_len, keys, sigs, prefix + b"\0") == [BAD(4)] * n
    assert verify_dev(torch, ed, msgs, msg_len, keys, sigs, prefix) == [0] * n


def test_bad_key_encodings(torch, ed):
    """y = p, y = p + 1, x = 0 with the sign bit set (y = 1 and y = -1), a y without a square root, the eight small-order encodings"""
    n = 16
    seeds, keys, msgs, sigs = signed_items(ed, n, 32, seed=5)
    no_root = next(y for y in range(2, 100) if R.decode(y.to_bytes(32, "little")) is None)
    bad = [R.P.to_bytes(32, "little"), (R.P + 1).to_bytes(32, "little"), (1 | 1 << 255).to_bytes(32, "little"),
           ((R.P - 1) | 1 << 255).to_bytes(32, "little"), no_root.to_bytes(32, "little"), ((1 << 255) - 1).to_bytes(32, "little"),
           bytes([0xFF] * 32)] + R.small_order_encodings()
    K = bad + [item(keys, 15, 32)]
    want = [R.status_word(R.verify_detail(K[i], item(msgs, i, 32), item(sigs, i, 64))) for i in range(n)]
    assert want == [BAD(2)] * 7 + [BAD(3)] * 8 + [0]
    assert verify_dev(torch, ed, msgs, 32, b"".join(K), sigs) == want


def test_large_batch_of_ballot_sized_messages(torch, ed):
    """20 011 items of 736 bytes under a roster of 499 keys, a tenth tampered (R, S, the message, the roster index, an index out of
    range): every untampered item accepted, every tampered one with the model's word, 64 of them through the model's full check"""
    n, msg_len, n_keys, prefix = 20011, 736, 499, b"precinct-count-2026"
    rseeds = rand(3, 32 * n_keys)
    roster = ed.keypairs(rseeds)
    rng = np.random.default_rng(8)
    idx = rng.integers(0, n_keys, n)
    seeds = np.frombuffer(rseeds, dtype=np.uint8).reshape(n_keys, 32)[idx].tobytes()
    msgs = np.frombuffer(rand(4, msg_len * n), dtype=np.uint8).reshape(n, msg_len).copy()
    sigs = np.frombuffer(ed.sign(seeds, msgs.tobytes(), msg_len, prefix), dtype=np.uint8).reshape(n, 64).copy()
    tampered = sorted(int(i) for i in rng.choice(n, n // 10, replace=False))
    use = [int(i) for i in idx]
    for k, i in enumerate(tampered):
        kind = k % 5
        if kind == 0:
            sigs[i, k % 32] ^= 1 << (k % 8)
        elif kind == 1:
            sigs[i, 32 + k % 32] ^= 1 << (k % 8)
        elif kind == 2:
            msgs[i, (7 * k) % msg_len] ^= 1 << (k % 8)
        elif kind == 3:
            use[i] = (use[i] + 1 + k % (n_keys - 1)) % n_keys
        else:
            use[i] = n_keys + k
    got = verify_dev(torch, ed, msgs.tobytes(), msg_len, roster, sigs.tobytes(), prefix, key_index=use)
    tset = set(tampered)
    want = [R.expected_status(item(roster, use[i], 32) if use[i] < n_keys else b"", b"", sigs[i].tobytes(), True, use[i] < n_keys) if i in tset else 0
            for i in range(n)]
    assert got == want
    assert sum(1 for w in want if w) == n // 10
    for i in list(range(0, n, n // 48))[:48] + tampered[:16]:              # the model in full
        full = BAD(R.BAD_INDEX) if use[i] >= n_keys else R.status_word(R.verify_detail(item(roster, use[i], 32), prefix + msgs[i].tobytes(), sigs[i].tobytes()))
        assert got[i] == full, i


# ------------------------------------------------------------------ chaining, forms of the entry
def test_status_in_passes_through_and_those_items_are_not_read(torch, ed):
    n, msg_len = 130, 48
    seeds, keys, msgs, sigs = signed_items(ed, n, msg_len, seed=21)
    status_in = [0] * n
    idx = list(range(n))
    s, m = bytearray(sigs), bytearray(msgs)
    for i in (0, 5, 63, 64, 129):
        status_in[i] = 0x00000406 + i * 0x10000
        s[64 * i:64 * i + 64] = b"\xFF" * 64                  # S far above l, R garbage
        m[msg_len * i:msg_len * (i + 1)] = b"\xEE" * msg_len
        idx[i] = 0xFFFFFFF0                                   # far out of the roster
    s[64 * 7] ^= 1                                            # and one genuine failure beside them
    want = list(status_in)
    want[7] = BAD(4)
    for alias in (False, True):
        assert verify_dev(torch, ed, bytes(m), msg_len, keys, bytes(s), key_index=idx, status_in=status_in, alias=alias) == want
    assert ed.verify(bytes(m), msg_len, keys, bytes(s), key_index=idx, status_in=status_in) == want


def test_roster_form_equals_per_item_keys_host_equals_device_on_a_caller_stream(torch, ed):
    n, msg_len, prefix = 200, 33, b"p"
    seeds, keys, msgs, sigs = signed_items(ed, n, msg_len, prefix, seed=31)
    sigs = bytearray(sigs)
    for i in range(0, n, 9):
        sigs[64 * i + 40] ^= 4
    sigs = bytes(sigs)
    perm = np.random.default_rng(1).permutation(n)
    roster = b"".join(item(keys, int(j), 32) for j in perm)
    inv = [0] * n
    for pos, j in enumerate(perm):
        inv[int(j)] = pos
    a = verify_dev(torch, ed, msgs, msg_len, keys, sigs, prefix)
    s = torch.cuda.Stream()
    b = verify_dev(torch, ed, msgs, msg_len, roster, sigs, prefix, key_index=inv, stream=s.cuda_stream)
    assert a == b == ed.verify(msgs, msg_len, roster, sigs, prefix, key_index=inv)
    assert [i for i, w in enumerate(a) if w] == list(range(0, n, 9))
    # a stride above the length, the gap poisoned
    stride = msg_len + 11
    wide = bytearray(b"\xEE" * (stride * n))
    for i in range(n):
        wide[i * stride:i * stride + msg_len] = item(msgs, i, msg_len)
    assert verify_dev(torch, ed, bytes(wide)[: (n - 1) * stride + msg_len], msg_len, keys, sigs, prefix, stride=stride) == a


def test_n_zero_and_every_refusal(torch, eg, ed):
    C = __import__("ctypes")
    lib, h = eg._load(), ed.ctx._h
    assert ed.verify(b"", 10, b"", b"") == [] and ed.keypairs(b"") == b"" and ed.sign(b"", b"", 4) == b"" and ed.sha512(b"", 4, n=0) == b""
    assert ed.verify_scratch_bytes(0) == 0
    ed.verify_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    n, msg_len = 4, 20
    seeds, keys, msgs, sigs = signed_items(ed, n, msg_len, seed=41)
    need = ed.verify_scratch_bytes(n)
    bufs = dict(m=dev(torch, msgs), k=dev(torch, keys), s=dev(torch, sigs), o=torch.zeros(n, dtype=torch.int32, device="cuda"),
                x=torch.zeros(need, dtype=torch.uint8, device="cuda"), i=u32(torch, [0, 1, 2, 3]))
    P = {k: v.data_ptr() for k, v in bufs.items()}

    def call(n=n, m=P["m"], stride=msg_len, length=msg_len, prefix=b"ab", plen=None, k=P["k"], n_keys=n, i=0, s=P["s"], o=P["o"], x=P["x"], xb=need):
        return lib.eg_ed25519_verify_device(h, n, m or None, stride, length, prefix, len(prefix or b"") if plen is None else plen, k or None, n_keys,
                                            i or None, s or None, None, o or None, x or None, xb, None)

    assert call() == 0
    torch.cuda.synchronize()
    assert as_u32(bufs["o"]) == [BAD(4)] * n                  # (signed without the prefix)
    BAD_ARG = -3
    assert lib.eg_ed25519_verify_device(None, n, P["m"], msg_len, msg_len, None, 0, P["k"], n, None, P["s"], None, P["o"], P["x"], need, None) == BAD_ARG
    for kw in (dict(m=0), dict(k=0), dict(s=0), dict(o=0), dict(x=0), dict(prefix=b"a" * 256), dict(prefix=None, plen=1), dict(stride=msg_len - 1),
               dict(n=1 << 31), dict(n_keys=0, i=P["i"]), dict(n_keys=n + 1), dict(n_keys=n - 1), dict(xb=need - 1), dict(k=P["k"] + 1),
               dict(s=P["s"] + 2), dict(o=P["o"] + 1)):
        assert call(**kw) == BAD_ARG, kw
        assert eg._load().eg_last_error()
    assert call(prefix=b"a" * 255) == 0 and call(n_keys=9, i=P["i"], k=P["k"]) == 0 and call(m=0, length=0, stride=0) == 0
    torch.cuda.synchronize()
    # host forms
    assert lib.eg_ed25519_verify_batch(h, n, msgs, msg_len, msg_len, None, 0, keys, n - 1, None, sigs, None, (C.c_uint32 * n)()) == BAD_ARG
    assert lib.eg_ed25519_verify_batch(h, n, msgs, msg_len, msg_len, None, 0, None, n, None, sigs, None, None) == BAD_ARG
    assert lib.eg_ed25519_sign_batch(h, n, None, msgs, msg_len, msg_len, None, 0, None) == BAD_ARG
    assert lib.eg_ed25519_sign_batch(h, n, seeds, msgs, msg_len - 1, msg_len, None, 0, C.create_string_buffer(64 * n)) == BAD_ARG
    assert lib.eg_ed25519_sign_batch(h, n, seeds, msgs, msg_len, msg_len, None, 3, C.create_string_buffer(64 * n)) == BAD_ARG
    assert lib.eg_ed25519_keypair_batch(h, n, None, None) == BAD_ARG and lib.eg_ed25519_keypair_batch(None, 0, None, None) == BAD_ARG
    assert lib.eg_sha512_batch(h, n, msgs, msg_len, msg_len, b"x" * 256, 256, C.create_string_buffer(64 * n)) == BAD_ARG
    assert lib.eg_sha512_batch(h, n, None, msg_len, msg_len, None, 0, C.create_string_buffer(64 * n)) == BAD_ARG
    assert lib.eg_sha512_batch(h, n, msgs, msg_len, msg_len, None, 0, None) == BAD_ARG
    assert lib.eg_ed25519_verify_scratch_bytes(None, 5) == 0 and lib.eg_ed25519_verify_scratch_bytes(h, 1 << 31) == 0


# ------------------------------------------------------------------ with the ballot pipeline
@pytest.fixture(scope="module")
def election(eg, ctx, oracle):
    pk = oracle.keypair_from_seed(12345)[1]
    return eg.ChoiceParams(ctx, pk, 5, True)


def test_a_pass_beside_a_verifying_thread(torch, ed, election):
    """two threads check signatures while a third verifies ballots on the same context: the pass takes no lock and no workspace of it"""
    p, n = election, 1500
    size = p.ballot_size
    d = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(808, 0, n, d.data_ptr())
    p.ctx.synchronize()
    ballots = bytes(d.cpu().numpy())
    seeds = rand(51, 32 * n)
    keys, sigs = ed.keypairs(seeds), bytearray(ed.sign(seeds, ballots, size, b"e"))
    for i in range(0, n, 50):
        sigs[64 * i + 1] ^= 8
    sigs = bytes(sigs)
    want = [BAD(4) if i % 50 == 0 else 0 for i in range(n)]
    errors, results = [], {}

    def signer(k):
        try:
            s = torch.cuda.Stream()
            results[k] = [verify_dev(torch, ed, ballots, size, keys, sigs, b"e", stream=s.cuda_stream) for _ in range(2)]
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    def verifier():
        try:
            s = torch.cuda.Stream()
            st = torch.full((n,), 9, dtype=torch.int32, device="cuda")
            for _ in range(3):
                p.verify_batch_device(n, d.data_ptr(), st.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            results["status"] = st.cpu().tolist()
        except Exception as e:           # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=signer, args=(0,)), threading.Thread(target=signer, args=(1,)), threading.Thread(target=verifier)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    p.tally_reset()
    assert not errors, errors
    assert results["status"] == [0] * n
    assert all(run == want for k in (0, 1) for run in results[k])


def test_end_to_end_forged_envelopes_stay_out_of_the_tally(torch, ed, election):
    """300 generated ballots signed under a roster; 20 envelopes forged (a wrong roster index, a flipped bit); signature pass ->
    verify_batch_device -> grouped tally over the chained status: byte for byte the verify entry's own tally of the other 280"""
    p, n, prefix = election, 300, b"election-42"
    size = p.ballot_size
    d = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(9191, 0, n, d.data_ptr())
    p.ctx.synchronize()
    ballots = bytes(d.cpu().numpy())
    seeds = rand(61, 32 * n)
    roster, sigs = ed.keypairs(seeds), bytearray(ed.sign(seeds, ballots, size, prefix))
    idx = list(range(n))
    forged = [(13 * i + 2) % n for i in range(20)]
    for k, b in enumerate(forged):
        if k % 2:
            idx[b] = (b + 1) % n
        else:
            sigs[64 * b + k] ^= 1
    sig_status = ed.verify(ballots, size, roster, bytes(sigs), prefix, key_index=idx)
    assert [b for b in range(n) if sig_status[b]] == sorted(forged) and all(sig_status[b] == BAD(4) for b in forged)
    status, _ = p.verify_batch(ballots)
    assert status == [0] * n                                          # the ballots themselves are all valid: only the envelope tells
    p.tally_reset()
    chained = [s or v for s, v in zip(sig_status, status)]
    tallies, counts = p.tally_grouped(ballots, chained, [0] * n, 1)
    kept = b"".join(item(ballots, b, size) for b in range(n) if b not in forged)
    _, tally_280 = p.verify_batch(kept)
    p.tally_reset()
    assert counts == [280] and tallies == tally_280


def test_cpp_voting_example_with_signed_envelopes(tmp_path):
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "voting.cpp"),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    out = subprocess.run([str(exe), "--signed", "5", "100", "5", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "5 forged envelopes: the signature pass refused 5 of 100" in out.stdout
    assert "the forgeries, and only they, are left out of the tally" in out.stdout
    assert "OK: the decrypted totals equal the expected ones" in out.stdout


# ------------------------------------------------------------------ a loose guard (the operation count puts the pass near a tenth)
def test_the_signature_pass_is_cheaper_than_verifying_the_ballots(torch, ed, election):
    """the pass over 2^16 five-option ballots (736 bytes) takes less time than eg_verify_choice_batch_device over the same ballots in the
    same process (warm, median of three, HIP events): a signature is one double-base product and seven SHA-512 blocks, a ballot 22
    products and their tables."""
    p, n = election, 1 << 16
    size = p.ballot_size
    assert size == 736
    d = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(4242, 0, n, d.data_ptr())
    p.ctx.synchronize()
    d_seeds = dev(torch, rand(71, 32 * n))
    d_keys = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    d_sigs = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ed.keypairs_device(n, d_seeds.data_ptr(), d_keys.data_ptr(), stream=stream)
    ed.sign_device(n, d_seeds.data_ptr(), d.data_ptr(), size, size, d_sigs.data_ptr(), stream=stream)
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    sig_status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    need = ed.verify_scratch_bytes(n)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")

    def timed(fn):
        ms = []
        for _ in range(4):                       # the first round warms up
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms[1:])

    verify_ms = timed(lambda: p.verify_batch_device(n, d.data_ptr(), status.data_ptr(), stream=stream))
    sig_ms = timed(lambda: ed.verify_device(n, d.data_ptr(), size, size, d_keys.data_ptr(), n, d_sigs.data_ptr(), sig_status.data_ptr(),
                                            scratch.data_ptr(), need, stream=stream))
    print(f"n = 2^16: signature pass {sig_ms:.3f} ms, batch verify {verify_ms:.3f} ms, ratio {sig_ms / verify_ms:.3f}")
    assert int(status.abs().sum().item()) == 0 and int(sig_status.abs().sum().item()) == 0
    assert sig_ms < verify_ms
    p.tally_reset()
