#!/usr/bin/env python3
"""Developer probe (not the benchmark): rates of the five single-item provers and of the matching verifiers in ONE process.
2^20 items of each kind in device memory: eg_proof_prove_batch_device / eg_share_prove_batch_device, then eg_verify_proof_batch_device
on the items just made (every one must be accepted), each timed with HIP events on both sides of every step, one warm-up step (it
also sizes the workspaces and builds the wide comb tables) and then `steps` timed ones; median.  Beside them the rate of what the GPU
provers replace as a source of test items: the oracle's prover on ONE thread of this box.  Nothing here is gated - these kernels had not
been measured before; the numbers are a record.  Writes profiles/r08_proof_provers.txt.
usage: proof_prove_probe.py [log2_n = 20] [steps = 8]"""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

import elastic_elgamal_amd as eg
from oracle import oracle as o

n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 20)
steps = max(5, int(sys.argv[2]) if len(sys.argv) > 2 else 8)
L = 2**252 + 27742317777372353535851937790883648493
sk, pk, _ = o.keypair_from_seed(12345)
ctx = eg.Context(0)
_, sclk = ctx.selfbench_fmul(1.0)


def timed(step):
    step()                                      # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return n / (ms[len(ms) // 2] * 1e-3), ms


def oracle_rate(make, count):
    t0 = time.perf_counter()
    for i in range(count):
        make(i)
    return count / (time.perf_counter() - t0)


k = o.PublicKey(pk)
pr = o.PreparedRange(100)
share_secret = (0x1234567 * 0x89ABCDEF123457) % L
share_key = o.point_mul_generator(share_secret.to_bytes(32, "little"))
d_status = torch.empty(n, dtype=torch.int32, device="cuda")
d_zero_items = None
lines = []
for name in ("zero", "bool", "range100", "sumsq5", "share"):
    if name == "zero":
        ver, d_in = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.ZERO), None
        slow = oracle_rate(lambda i: k.encrypt_zero(o.rng_from_u64(i)), 2000)
    elif name == "bool":
        ver, d_in = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.BOOL), torch.randint(0, 2, (n,), dtype=torch.int64, device="cuda")
        slow = oracle_rate(lambda i: k.encrypt_bool(bool(i & 1), o.rng_from_u64(i)), 1000)
    elif name == "range100":
        ver, d_in = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.RANGE, 100), torch.randint(0, 100, (n,), dtype=torch.int64, device="cuda")
        slow = oracle_rate(lambda i: k.encrypt_range(pr, i % 100, o.rng_from_u64(i)), 200)
    elif name == "sumsq5":
        ver, d_in = eg.SumOfSquaresVerifier(ctx, pk, 5, b"test"), torch.randint(0, 1000, (n, 5), dtype=torch.int64, device="cuda")
        slow = oracle_rate(lambda i: k.sumsq_snapshot([i % 7, 1, 2, 3, 4], o.rng_from_u64(i)), 200)
    else:
        ver = eg.DecryptionShareVerifier(ctx, pk, 3, 2, 0, share_key)
        d_in = d_zero_items.view(n, 128)[:, :32].contiguous()          # the random elements of the zero encryptions made above
        r0 = bytes(d_in[0].cpu().numpy().tobytes())
        slow = oracle_rate(lambda i: o.decryption_share_new(share_secret.to_bytes(32, "little"), r0, 3, 2, pk, 0, o.rng_from_u64(i)), 2000)
    d_items = torch.empty(n * ver.item_size, dtype=torch.uint8, device="cuda")
    if name == "share":
        d_ok = torch.empty(n, dtype=torch.uint8, device="cuda")
        prove = lambda: ver.prove_device(share_secret.to_bytes(32, "little"), 7, 0, n, d_in.data_ptr(), d_items.data_ptr(), d_ok.data_ptr())
    else:
        prove = lambda: ver.prove_device(7, 0, n, d_in.data_ptr() if d_in is not None else 0, d_items.data_ptr())
    p_rate, p_ms = timed(prove)
    v_rate, v_ms = timed(lambda: ver.verify_device(n, d_items.data_ptr(), d_status.data_ptr()))
    accepted = int((d_status == 0).sum())
    assert accepted == n, f"{name}: {accepted} of {n} accepted"
    if name == "share":
        assert int(d_ok.sum()) == n
    if name == "zero":
        d_zero_items = d_items
    lines += [f"{name}_item_bytes {ver.item_size}",
              f"{name}_prove_items_per_s {p_rate:.0f}",
              f"{name}_verify_items_per_s {v_rate:.0f}",
              f"{name}_oracle_prove_one_thread_items_per_s {slow:.0f}",
              f"{name}_prove_step_ms " + " ".join(f"{x:.2f}" for x in p_ms),
              f"{name}_verify_step_ms " + " ".join(f"{x:.2f}" for x in v_ms)]
    ver.close()
    if name != "zero":
        del d_items

head = [f"# tools/proof_prove_probe.py {n.bit_length() - 1} {steps}   [{ctx.name}]",
        f"# eg_proof_prove_batch_device / eg_share_prove_batch_device, then eg_verify_proof_batch_device on the items just made (all accepted):",
        f"# n = {n} items in device memory, median of {steps} steps after one warm-up step, HIP events; wide comb tables {ctx.comb_table_bits()[1]} bits;",
        "# oracle_prove_one_thread = the CPU checker's prover on one thread of the same box, the source of such items before;",
        "# a first measurement of these kernels: recorded, not gated",
        f"sclk_mhz {sclk:.0f}"]
text = "\n".join(head + lines) + "\n"
(ROOT / "profiles" / "r08_proof_provers.txt").write_text(text)
print(text, end="")
ctx.close()
