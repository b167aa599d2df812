#!/usr/bin/env python3
"""Developer probe (not the benchmark): rate of the commitment-equivalence verifier against the zero-encryption verifier in ONE process.
2^20 items of each kind in device memory, eg_verify_proof_batch_device timed with HIP events on both sides of every step, one warm-up
step (it also builds the wide comb tables) and then `steps` timed ones.  Commitment-equivalence items come from the GPU prover; the
library has no zero-encryption prover, so 4096 distinct valid items from the CPU checker are tiled (the accept path does the same
work for every item).  Writes items/s of both, their ratio and the shader clock to profiles/r07_commit_equiv.txt.
usage: commit_equiv_probe.py [log2_n = 20] [steps = 8]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

import elastic_elgamal_amd as eg
from oracle import oracle as o

n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 20)
steps = max(5, int(sys.argv[2]) if len(sys.argv) > 2 else 8)
pk = bytes.fromhex("a6adb6e9c0ae8d54c26e6e56b5ccd7a16bb0e1951abe4d7ee7028e3d4eca8531")
h = bytes([140, 146, 64, 180, 86, 169, 230, 220, 101, 195, 119, 161, 4, 141, 116, 95, 148, 160, 140, 219, 127, 68, 203, 205, 123, 70,
           243, 64, 72, 135, 17, 52])          # the Bulletproofs blinding base
ctx = eg.Context(0)
_, sclk = ctx.selfbench_fmul(1.0)


def timed(ver, d_items, d_status):
    ver.verify_device(n, d_items.data_ptr(), d_status.data_ptr())          # warm-up: workspace, wide comb tables
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ver.verify_device(n, d_items.data_ptr(), d_status.data_ptr())
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    accepted = int((d_status == 0).sum())
    assert accepted == n, f"{accepted} of {n} accepted"
    ms.sort()
    return n / (ms[len(ms) // 2] * 1e-3), ms


ce = eg.CommitmentEquivalenceVerifier(ctx, pk, h, b"probe")
d_vals = torch.randint(0, 2**62, (n,), dtype=torch.int64, device="cuda")
d_items = torch.empty(n * ce.item_size, dtype=torch.uint8, device="cuda")
d_status = torch.empty(n, dtype=torch.int32, device="cuda")
ce.prove_device(7, 0, n, d_vals.data_ptr(), d_items.data_ptr())
ctx.synchronize()
ce_rate, ce_ms = timed(ce, d_items, d_status)
ce.close()
del d_items

z = eg.PublicKeyVerifier(ctx, pk, eg.PublicKeyVerifier.ZERO)
k, rng = o.PublicKey(pk), o.rng_from_u64(7)
distinct = b"".join(k.encrypt_zero(rng) for _ in range(4096))
d_zero = torch.frombuffer(bytearray(distinct), dtype=torch.uint8).cuda().repeat(n // 4096)
z_rate, z_ms = timed(z, d_zero, d_status)
z.close()

lines = [f"# tools/commit_equiv_probe.py {n.bit_length() - 1} {steps}   [{ctx.name}]",
         f"# eg_verify_proof_batch_device over n = {n} items in device memory, median of {steps} steps after one warm-up step, HIP events;",
         f"# wide comb tables {ctx.comb_table_bits()[1]} bits; shader clock from eg_selfbench_fmul before the runs",
         f"commit_equiv_items_per_s {ce_rate:.0f}",
         f"zero_encryption_items_per_s {z_rate:.0f}",
         f"ratio {ce_rate / z_rate:.4f}",
         f"sclk_mhz {sclk:.0f}",
         "commit_equiv_step_ms " + " ".join(f"{x:.2f}" for x in ce_ms),
         "zero_encryption_step_ms " + " ".join(f"{x:.2f}" for x in z_ms)]
text = "\n".join(lines) + "\n"
(ROOT / "profiles" / "r07_commit_equiv.txt").write_text(text)
print(text, end="")
ctx.close()
