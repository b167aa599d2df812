#!/usr/bin/env python3
"""Developer probe: what the receipt log (eg_merkle_leaves_device / _tree_device / _paths_device / _check_device) costs beside the verify
call it follows and beside the only route there was before it.  Device-resident arrays, HIP events, median of 5 after a warm-up call:
  leaf pass   2^16 and 2^20 five-option ballots with their 64-byte signature slot as the extra, every output asked for and the append
  tree        2^16, 2^20 and 10^7 leaves, with the node store
  paths       one receipt per leaf of up to 2^20 requested leaves (random indices)        check   the same receipts against the root
  verify      eg_verify_choice_batch_device over the same ballots, in the same process
  detour      the tree by one eg_sha512_batch_device call per level, with a torch gather in between that builds the 65-byte node
              messages (0x01 and the two children) and a slice that keeps the first 32 bytes of each digest; an odd last node is copied
A first measurement, one run each: recorded, not gated.

  merkle_probe.py               writes profiles/r19_receipt_log.txt
  merkle_probe.py --out PATH    writes PATH"""
import hashlib
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

import elastic_elgamal_amd as eg

args = sys.argv[1:]
OUT = Path(args[args.index("--out") + 1]) if "--out" in args else ROOT / "profiles" / "r19_receipt_log.txt"
BALLOTS = [int(a) for a in args[args.index("--ballots") + 1].split(",")] if "--ballots" in args else [1 << 16, 1 << 20]
TREES = [int(a) for a in args[args.index("--trees") + 1].split(",")] if "--trees" in args else [1 << 16, 1 << 20, 10 ** 7]
pk = bytes.fromhex("a6adb6e9c0ae8d54c26e6e56b5ccd7a16bb0e1951abe4d7ee7028e3d4eca8531")
ctx = eg.Context(0)
ed, rl = eg.Ed25519(ctx), eg.ReceiptLog(ctx, b"election-19")
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


say(f"device: {ctx.name}; H = the first 32 bytes of SHA-512; times in ms, one run")
verify_at = {}
say(f"{'ballots':>8s} {'bytes':>6s} {'leaf pass':>9s} {'Mleaf/s':>8s} {'GB/s':>6s} {'tree':>8s} {'verify':>9s} {'(leaf+tree)/verify':>18s}")
for n in BALLOTS:
    params = eg.ChoiceParams(ctx, pk, 5, True)
    size = params.ballot_size
    ballots, status = zeros(n * size), zeros(n, torch.int32)
    params.encrypt_batch_device(4242, 0, n, ballots.data_ptr())
    verify_ms = event_ms(lambda: params.verify_batch_device(n, ballots.data_ptr(), status.data_ptr(), stream=stream), reps=3)
    assert int(status.abs().sum().item()) == 0
    params.tally_reset()
    sigs = torch.randint(0, 256, (64 * n,), dtype=torch.uint8, device="cuda")
    index, out, log, count, found = zeros(n, torch.int64), zeros(32 * n), zeros(32 * n), zeros(1, torch.int64), zeros(2, torch.int32)
    need = rl.leaves_scratch_bytes(n)
    scratch = zeros(need)
    leaf_ms = event_ms(lambda: rl.leaves_device(n, ballots.data_ptr(), size, size, index.data_ptr(), found.data_ptr(), scratch.data_ptr(), need,
                                                d_extra=sigs.data_ptr(), extra_stride=64, extra_len=64, d_status_in=status.data_ptr(),
                                                d_leaves_out=out.data_ptr(), d_log=log.data_ptr(), log_cap=n, d_log_count=count.data_ptr(), stream=stream))
    assert found.cpu().tolist() == [n, 0] and int(count.item()) == n
    b = n - 1                                                                # one leaf against hashlib
    want = hashlib.sha512(b"\x00election-19" + ballots[b * size:(b + 1) * size].cpu().numpy().tobytes() + sigs[64 * b:].cpu().numpy().tobytes()).digest()[:32]
    assert log[32 * b:32 * b + 32].cpu().numpy().tobytes() == want
    root, nodes = zeros(32), zeros(rl.nodes_bytes(n))
    tree_ms = event_ms(lambda: rl.tree_device(n, log.data_ptr(), root.data_ptr(), nodes.data_ptr(), stream=stream))
    verify_at[n] = verify_ms
    say(f"{n:8d} {size:6d} {leaf_ms:9.3f} {n / leaf_ms / 1e3:8.1f} {n * (size + 64) / leaf_ms / 1e6:6.1f} {tree_ms:8.3f} {verify_ms:9.3f} "
        f"{(leaf_ms + tree_ms) / verify_ms:18.4f}")
    del ballots, status, sigs, index, out, log, scratch, root, nodes, params
    torch.cuda.empty_cache()

say(f"{'leaves':>9s} {'depth':>5s} {'tree':>8s} {'Mnode/s':>8s} {'launches':>8s} {'detour':>9s} {'detour/tree':>11s} {'receipts':>9s} {'paths':>8s} {'check':>8s} "
    f"{'Mcheck/s':>8s} {'tree/verify':>11s}")
for n in TREES:
    log = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, device="cuda")
    depth = rl.depth(n)
    root, nodes = zeros(32), zeros(rl.nodes_bytes(n))
    tree_ms = event_ms(lambda: rl.tree_device(n, log.data_ptr(), root.data_ptr(), nodes.data_ptr(), stream=stream))
    one = torch.ones(1, dtype=torch.uint8, device="cuda")

    def detour():
        level = log.view(-1, 32)
        while level.shape[0] > 1:
            pairs = level.shape[0] // 2
            msgs = torch.empty((pairs, 65), dtype=torch.uint8, device="cuda")
            msgs[:, 0] = one
            msgs[:, 1:] = level[: 2 * pairs].reshape(pairs, 64)
            digests = torch.empty((pairs, 64), dtype=torch.uint8, device="cuda")
            ed.sha512_device(pairs, msgs.data_ptr(), 65, 65, digests.data_ptr(), stream=stream)
            up = digests[:, :32]
            level = torch.cat([up, level[2 * pairs:]]) if level.shape[0] & 1 else up.contiguous()
        return level

    detour_ms = event_ms(detour, reps=3)
    assert detour().view(-1).cpu().numpy().tobytes() == root.cpu().numpy().tobytes(), "the detour and the tree kernel disagree on the root"
    m = min(n, 1 << 20)
    index = torch.randint(0, n, (m,), dtype=torch.int64, device="cuda")
    paths, lens = zeros(m * 32 * depth), zeros(m, torch.int32)
    paths_ms = event_ms(lambda: rl.paths_device(m, index.data_ptr(), n, log.data_ptr(), nodes.data_ptr(), paths.data_ptr(), lens.data_ptr(), stream=stream))
    leaves = log.view(-1, 32)[index].contiguous()
    verdict, found = zeros(m, torch.int32), zeros(3, torch.int32)
    check_ms = event_ms(lambda: rl.check_device(m, index.data_ptr(), leaves.data_ptr(), paths.data_ptr(), 32 * depth, lens.data_ptr(), n, root.data_ptr(),
                                                verdict.data_ptr(), found.data_ptr(), stream=stream))
    assert found.cpu().tolist() == [0, 0, 0] and int(verdict.abs().sum().item()) == 0, "a receipt the library issued is not proven"
    beside = verify_at.get(n)
    say(f"{n:9d} {depth:5d} {tree_ms:8.3f} {(n - 1) / tree_ms / 1e3:8.1f} {-(-depth // 10):8d} {detour_ms:9.3f} {detour_ms / tree_ms:11.1f} {m:9d} {paths_ms:8.3f} "
        f"{check_ms:8.3f} {m / check_ms / 1e3:8.1f} " + (f"{tree_ms / beside:11.5f}" if beside else f"{'-':>11s}"))
    del log, root, nodes, index, paths, lens, leaves, verdict, found
    torch.cuda.empty_cache()

OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
print(f"wrote {OUT}")
