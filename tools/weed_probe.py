#!/usr/bin/env python3
"""Developer probe: what ballot weeding (eg_choice_weed_device) costs beside the verification it follows.
Device-resident 5-option single-choice ballots of the GPU generator, n = 2^16 and 2^20, with 0 %, 1 % and 100 % duplicates (whole copies
of an earlier ballot; 100 %: every ballot is a copy of ballot 0), beside a board of 0 and of 5 x 10^6 ciphertexts (random bytes: no hits).
Time of the pass alone, with the append (HIP events, median of 5 after a warm-up call), beside the batch verify call of the same ballots
in the same process and beside a torch.unique(dim=0) over the same keys (gathered into one tensor first; gather and unique timed
separately; the board is not part of that detour).  A first measurement, one run: recorded, not gated.

  weed_probe.py               writes profiles/r15_weed.txt
  weed_probe.py --out PATH    writes PATH"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

import elastic_elgamal_amd as eg

args = sys.argv[1:]
OUT = Path(args[args.index("--out") + 1]) if "--out" in args else ROOT / "profiles" / "r15_weed.txt"
pk = bytes.fromhex("a6adb6e9c0ae8d54c26e6e56b5ccd7a16bb0e1951abe4d7ee7028e3d4eca8531")
ctx = eg.Context(0)
p = eg.ChoiceParams(ctx, pk, 5, True)
K, SIZE = 5, p.ballot_size
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


say(f"device: {ctx.name}; 5-option single-choice ballots of {SIZE} bytes, 5 keys of 64 bytes each; times in ms, one run")
say(f"{'n':>8s} {'dups':>5s} {'board':>8s} {'weed':>9s} {'verify':>9s} {'verify/weed':>11s} {'flagged':>8s} {'appended':>9s} {'scratch MB':>10s} "
    f"{'gather':>8s} {'unique':>9s}")
board_big = torch.randint(0, 256, (5_000_000 * 64,), dtype=torch.uint8, device="cuda")
for n in (1 << 16, 1 << 20):
    base = torch.zeros(n * SIZE, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(4242, 0, n, base.data_ptr())
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    verify_ms = event_ms(lambda: p.verify_batch_device(n, base.data_ptr(), status.data_ptr(), stream=stream))
    assert int(status.abs().sum().item()) == 0
    rng = np.random.default_rng(n)
    for dups in (0, 1, 100):
        d = base.clone().view(n, SIZE)
        if dups == 100:
            d[1:] = d[0]
            want = n - 1
        elif dups:
            which = np.sort(rng.choice(np.arange(1, n), n // 100, replace=False))
            src = (rng.random(which.size) * which).astype(np.int64)          # an earlier ballot each
            src = np.where(np.isin(src, which), 0, src)                      # ... that is an original itself
            d[torch.from_numpy(which).cuda()] = d[torch.from_numpy(src).cuda()]
            want = which.size
        else:
            want = 0
        d = d.view(-1)
        torch.cuda.synchronize()
        gather_ms = unique_ms = float("nan")
        for n_prior in (0, 5_000_000):
            cap = n_prior + n * K
            board = torch.empty(cap * 64, dtype=torch.uint8, device="cuda")
            board[: n_prior * 64] = board_big[: n_prior * 64]
            need = p.weed_scratch_bytes(n, n_prior)
            scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
            dup = torch.zeros(n, dtype=torch.int32, device="cuda")
            out = torch.zeros(n, dtype=torch.int32, device="cuda")
            found = torch.zeros(3, dtype=torch.int32, device="cuda")
            count = torch.zeros(1, dtype=torch.int64, device="cuda")
            seed = int(rng.integers(0, 1 << 62))
            ms = event_ms(lambda: p.weed_device(n, d.data_ptr(), status.data_ptr(), n_prior, board.data_ptr(), cap, seed, scratch.data_ptr(),
                                                dup.data_ptr(), found.data_ptr(), d_status_out=out.data_ptr(), d_board_count=count.data_ptr(),
                                                stream=stream))
            f = found.cpu().tolist()
            assert f == [0, want, 0], f
            assert int(count.item()) == n_prior + (n - want) * K
            if n_prior == 0:
                # the detour: the keys gathered into one [n K, 8] int64 tensor, then torch.unique over its rows
                keys = None

                def gather():
                    global keys
                    keys = d.view(n, SIZE)[:, : 64 * K].contiguous().view(n * K, 64).view(torch.int64)

                gather_ms = event_ms(gather, reps=3)
                uniq = None

                def unique():
                    global uniq
                    uniq = torch.unique(keys, dim=0)

                unique_ms = event_ms(unique, reps=1, warm=1)
                assert uniq.shape[0] == (n - want) * K
                del keys, uniq
            say(f"{n:8d} {dups:4d}% {n_prior:8d} {ms:9.3f} {verify_ms:9.3f} {verify_ms / ms:11.1f} {f[0] + f[1]:8d} {(n - want) * K:9d} "
                f"{need / 1e6:10.1f} {gather_ms:8.3f} {unique_ms:9.3f}")
            del board, scratch
        del d
    p.tally_reset()
    del base
say("gather / unique: the keys of the batch copied into one tensor and torch.unique(dim=0) over it (batch only, no board, no owner indices)")
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
