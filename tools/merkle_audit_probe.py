#!/usr/bin/env python3
"""Developer probe: what the audit entries of the receipt log (eg_merkle_heads_device / _consistency_device / _consistency_check_device)
cost beside the inclusion check and the tree they read.  Device-resident arrays, HIP events, median of 5 after a warm-up call, all in
one process:
  heads        2^16 and 2^20 earlier sizes (random in 1 .. N) against a log of N = 2^20 and 10^7 leaves
  consistency  their proofs out of the node store          cons check   the same proofs against the root
  check        eg_merkle_check_device over as many receipts of the same log        tree   eg_merkle_tree_device with the node store
A first measurement, one run each: recorded, not gated.

  merkle_audit_probe.py               writes profiles/r20_log_audit.txt
  merkle_audit_probe.py --out PATH    writes PATH"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

import elastic_elgamal_amd as eg

args = sys.argv[1:]
OUT = Path(args[args.index("--out") + 1]) if "--out" in args else ROOT / "profiles" / "r20_log_audit.txt"
TREES = [int(a) for a in args[args.index("--trees") + 1].split(",")] if "--trees" in args else [1 << 20, 10 ** 7]
HEADS = [int(a) for a in args[args.index("--heads") + 1].split(",")] if "--heads" in args else [1 << 16, 1 << 20]
ctx = eg.Context(0)
rl = eg.ReceiptLog(ctx, b"election-20")
stream = torch.cuda.current_stream().cuda_stream
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def event_ms(fn, reps=5, warm=1):
    ts = []
    for k in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= warm:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def zeros(n, dtype=torch.uint8):
    return torch.zeros(max(n, 1), dtype=dtype, device="cuda")


say(f"device: {ctx.name}; H = the first 32 bytes of SHA-512; times in ms, median of 5 warm calls, one run")
say(f"{'leaves':>9s} {'depth':>5s} {'tree':>8s} {'items':>8s} {'heads':>8s} {'Mhead/s':>8s} {'consist.':>8s} {'GB/s':>6s} {'cons chk':>8s} {'Mchk/s':>7s} "
    f"{'incl chk':>8s} {'cons/incl':>9s} {'entries':>8s}")
for n in TREES:
    log = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, device="cuda")
    depth = rl.depth(n)
    root, nodes = zeros(32), zeros(rl.nodes_bytes(n))
    tree_ms = event_ms(lambda: rl.tree_device(n, log.data_ptr(), root.data_ptr(), nodes.data_ptr(), stream=stream))
    for m in HEADS:
        old = torch.randint(1, n + 1, (m,), dtype=torch.int64, device="cuda")
        row = 32 * (depth + 1)
        heads, hfound = zeros(32 * m), zeros(1, torch.int32)
        heads_ms = event_ms(lambda: rl.heads_device(m, old.data_ptr(), n, log.data_ptr(), nodes.data_ptr(), heads.data_ptr(), hfound.data_ptr(), stream=stream))
        proofs, lens = zeros(m * row), zeros(m, torch.int32)
        cons_ms = event_ms(lambda: rl.consistency_device(m, old.data_ptr(), n, log.data_ptr(), nodes.data_ptr(), proofs.data_ptr(), lens.data_ptr(), stream=stream))
        verdict, found = zeros(m, torch.int32), zeros(4, torch.int32)
        check_ms = event_ms(lambda: rl.consistency_check_device(m, old.data_ptr(), heads.data_ptr(), proofs.data_ptr(), row, lens.data_ptr(), n, root.data_ptr(),
                                                                verdict.data_ptr(), found.data_ptr(), stream=stream))
        assert hfound.cpu().tolist() == [0] and found.cpu().tolist() == [0, 0, 0, 0] and int(verdict.abs().sum().item()) == 0, \
            "a consistency proof the library issued is not proven"
        entries = float(lens.sum().item()) / m
        # as many receipts of the same log, beside
        index = torch.randint(0, n, (m,), dtype=torch.int64, device="cuda")
        paths, plens = zeros(m * 32 * depth), zeros(m, torch.int32)
        rl.paths_device(m, index.data_ptr(), n, log.data_ptr(), nodes.data_ptr(), paths.data_ptr(), plens.data_ptr(), stream=stream)
        leaves = log.view(-1, 32)[index].contiguous()
        v2, f2 = zeros(m, torch.int32), zeros(3, torch.int32)
        incl_ms = event_ms(lambda: rl.check_device(m, index.data_ptr(), leaves.data_ptr(), paths.data_ptr(), 32 * depth, plens.data_ptr(), n, root.data_ptr(),
                                                   v2.data_ptr(), f2.data_ptr(), stream=stream))
        assert f2.cpu().tolist() == [0, 0, 0], "a receipt the library issued is not proven"
        say(f"{n:9d} {depth:5d} {tree_ms:8.3f} {m:8d} {heads_ms:8.3f} {m / heads_ms / 1e3:8.1f} {cons_ms:8.3f} {m * row / cons_ms / 1e6:6.1f} {check_ms:8.3f} "
            f"{m / check_ms / 1e3:7.1f} {incl_ms:8.3f} {check_ms / incl_ms:9.2f} {entries:8.2f}")
        del old, heads, hfound, proofs, lens, verdict, found, index, paths, plens, leaves, v2, f2
        torch.cuda.empty_cache()
    del log, root, nodes
    torch.cuda.empty_cache()

OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
print(f"wrote {OUT}")
