#!/usr/bin/env python3
"""Developer probe: what growing the receipt log's tree by a batch (eg_merkle_grow_device) costs beside the full rebuild
(eg_merkle_tree_device with its node store) and beside the verify call of the batch.  Device-resident arrays, HIP events, median of 7
after two warm-up calls, all in one process:
  grow         a batch of 2^16 and 2^20 leaves onto boards of 2^20 and 10^7 leaves, and m == N (nothing appended)
  copy         grow at m == N: the copy launch plus at most one ragged tile per launch and the root, with the bytes the copy reads and
               writes per second as if it were the copy alone (a lower bound on the copy's rate).  m == N = 2^20 is the copy and the
               root and nothing else; m == N = 2^23 (268 MB) has one tile of 8 nodes beside them
  rebuild      eg_merkle_tree_device over the grown log          verify   the batch's verify call (five-option ballots)
The grown store is compared with the rebuilt one in every row.  A first measurement, one run each: recorded, not gated.

  merkle_grow_probe.py               writes profiles/r22_merkle_grow.txt
  merkle_grow_probe.py --out PATH    writes PATH"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

import elastic_elgamal_amd as eg

args = sys.argv[1:]
OUT = Path(args[args.index("--out") + 1]) if "--out" in args else ROOT / "profiles" / "r22_merkle_grow.txt"
BOARDS = [int(a) for a in args[args.index("--boards") + 1].split(",")] if "--boards" in args else [1 << 20, 10 ** 7]
BATCHES = [int(a) for a in args[args.index("--batches") + 1].split(",")] if "--batches" in args else [1 << 16, 1 << 20]
ctx = eg.Context(0)
rl = eg.ReceiptLog(ctx, b"election-22")
stream = torch.cuda.current_stream().cuda_stream
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def event_ms(fn, reps=7, warm=2):
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


def zeros(n):
    return torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")


def copied_nodes(m):
    """the nodes of the copy launch: on level L0 + s of launch L0 = 0, 10, 20 the first ((m >> L0) >> 10) << (10 - s)"""
    return sum(((m >> (l0 + 10)) << (10 - s)) for l0 in (0, 10, 20) for s in range(1, 11) if m >> (l0 + 10))


say(f"device: {ctx.name}; H = the first 32 bytes of SHA-512; times in ms, median of 7 calls after 2 warm-ups, one run")
verify_ms = {}
pk = bytes.fromhex("a6adb6e9c0ae8d54c26e6e56b5ccd7a16bb0e1951abe4d7ee7028e3d4eca8531")
for batch in BATCHES:
    params = eg.ChoiceParams(ctx, pk, 5, True)
    ballots, status = zeros(batch * params.ballot_size), torch.zeros(batch, dtype=torch.int32, device="cuda")
    params.encrypt_batch_device(2222, 0, batch, ballots.data_ptr())
    verify_ms[batch] = event_ms(lambda: params.verify_batch_device(batch, ballots.data_ptr(), status.data_ptr(), stream=stream), reps=3, warm=1)
    assert int(status.abs().sum().item()) == 0
    params.tally_reset()
    del ballots, status, params
    torch.cuda.empty_cache()
say(f"{'board m':>9s} {'batch':>8s} {'N':>9s} {'grow':>8s} {'rebuild':>8s} {'grow/reb':>8s} {'copied MB':>9s} {'hashed':>9s} {'verify':>8s} {'grow/ver':>8s}")
for m in BOARDS + [1 << 23]:
    for batch in (BATCHES if m in BOARDS else []) + [0]:            # m == N = 2^23: a copy, and ONE tile of 8 nodes at the third launch
        n = m + batch
        log = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, device="cuda")
        old, new, rebuilt, root, root2 = zeros(rl.nodes_bytes(m)), zeros(rl.nodes_bytes(n)), zeros(rl.nodes_bytes(n)), zeros(32), zeros(32)
        rl.tree_device(m, log.data_ptr(), root.data_ptr(), old.data_ptr(), stream=stream)
        tree_ms = event_ms(lambda: rl.tree_device(n, log.data_ptr(), root2.data_ptr(), rebuilt.data_ptr(), stream=stream))
        grow_ms = event_ms(lambda: rl.grow_device(m, old.data_ptr(), n, log.data_ptr(), new.data_ptr(), root.data_ptr(), stream=stream))
        torch.cuda.synchronize()
        assert torch.equal(new, rebuilt) and torch.equal(root, root2), "the grown store differs from the rebuilt one"
        copied = copied_nodes(m)
        hashed = rl.nodes_bytes(n) // 32 - copied
        ver = verify_ms.get(batch)
        say(f"{m:9d} {batch:8d} {n:9d} {grow_ms:8.3f} {tree_ms:8.3f} {grow_ms / tree_ms:8.3f} {copied * 32 / 1e6:9.1f} {hashed:9d} "
            + (f"{ver:8.2f} {grow_ms / ver:8.4f}" if ver else f"{'-':>8s} {'-':>8s}"))
        if batch == 0:
            say(f"{'':9s} m == N: the copy of {copied * 32 / 1e6:.1f} MB and {hashed} nodes of the ragged tiles in {grow_ms:.3f} ms: "
                f"{2 * copied * 32 / grow_ms / 1e6:.0f} GB/s read + written if it were the copy alone")
        del log, old, new, rebuilt, root, root2
        torch.cuda.empty_cache()

OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
print(f"wrote {OUT}")
