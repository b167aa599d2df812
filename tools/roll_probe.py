#!/usr/bin/env python3
"""Developer probe: what the voter-roll pass (eg_roll_cast_device / eg_roll_check_device) costs beside the passes it follows.
Device-resident arrays, n = 2^16 and 2^20 ballots against rosters of 2^20 and 10^7 keys, with every output asked for (status_out,
groups_out, weights_out, displaced).  Per row (HIP events, median of 5 after a warm-up call; the cast's time includes putting the prior
roll back with one device copy, whose time alone is the column `reset`):
  pattern   spread  one ballot per key (a random permutation of distinct keys)
            revote  spread with 1 % of the ballots re-voting under a key used earlier in the batch
            flood   every ballot under ONE key: every atomic of the claim kernel on one address
  prior     empty   a zero roll                      full    every key holds a word of an earlier sequence number (LAST: all displaced)
  cast      eg_roll_cast_device                      check   eg_roll_check_device against the roll the cast left
Beside them, in the same process, over as many items: the signature pass (eg_ed25519_verify_device, 32-byte messages) and the verify
entry (eg_verify_choice_batch_device, five-option ballots).  The flood rows against the signature pass decided that k_roll_claim got
its wave-level combine: profiles/r18_voter_roll.txt keeps the run without it (12.1 ms against 11.7 ms at 2^20) above the run with it.
A first measurement, one run each: recorded, not gated.

  roll_probe.py               writes profiles/r18_voter_roll.txt
  roll_probe.py --out PATH    writes PATH"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

import elastic_elgamal_amd as eg

args = sys.argv[1:]
OUT = Path(args[args.index("--out") + 1]) if "--out" in args else ROOT / "profiles" / "r18_voter_roll.txt"
SIZES = [int(a) for a in args[args.index("--sizes") + 1].split(",")] if "--sizes" in args else [1 << 16, 1 << 20]
ROSTERS = [int(a) for a in args[args.index("--rosters") + 1].split(",")] if "--rosters" in args else [1 << 20, 10 ** 7]
pk = bytes.fromhex("a6adb6e9c0ae8d54c26e6e56b5ccd7a16bb0e1951abe4d7ee7028e3d4eca8531")
ctx = eg.Context(0)
ed, vr = eg.Ed25519(ctx), eg.VoterRoll(ctx, eg.ROLL_LAST)
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


say(f"device: {ctx.name}; policy LAST; times in ms, one run")
beside = {}
for n in SIZES:
    msgs = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device="cuda")
    seeds = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device="cuda")
    keys, sigs, status = zeros(32 * n), zeros(64 * n), torch.full((n,), 7, dtype=torch.int32, device="cuda")
    need = ed.verify_scratch_bytes(n)
    scratch = zeros(need)
    ed.keypairs_device(n, seeds.data_ptr(), keys.data_ptr(), stream=stream)
    ed.sign_device(n, seeds.data_ptr(), msgs.data_ptr(), 32, 32, sigs.data_ptr(), stream=stream)
    sig_ms = event_ms(lambda: ed.verify_device(n, msgs.data_ptr(), 32, 32, keys.data_ptr(), n, sigs.data_ptr(), status.data_ptr(), scratch.data_ptr(), need,
                                               stream=stream))
    assert int(status.abs().sum().item()) == 0, "a signature of the GPU signer was refused"
    del msgs, seeds, keys, sigs, scratch
    params = eg.ChoiceParams(ctx, pk, 5, True)
    ballots, ballot_status = zeros(n * params.ballot_size), zeros(n, torch.int32)
    params.encrypt_batch_device(4242, 0, n, ballots.data_ptr())
    verify_ms = event_ms(lambda: params.verify_batch_device(n, ballots.data_ptr(), ballot_status.data_ptr(), stream=stream), reps=3)
    assert int(ballot_status.abs().sum().item()) == 0
    params.tally_reset()
    del ballots, params
    torch.cuda.empty_cache()
    beside[n] = (sig_ms, verify_ms)
    say(f"beside, n = {n}: signature pass {sig_ms:.3f} ms, verify entry {verify_ms:.3f} ms")

say(f"{'n':>8s} {'keys':>9s} {'pattern':>7s} {'prior':>6s} {'cast':>8s} {'reset':>7s} {'Mballot/s':>9s} {'check':>8s} {'cast/sig':>8s} {'cast/verify':>11s} "
    f"{'superseded':>10s} {'displaced':>9s} {'scratch MB':>10s}")
flood_at = {}
for n in SIZES:
    for n_keys in ROSTERS:
        groups = torch.randint(0, 1000, (n_keys,), dtype=torch.int32, device="cuda")
        weights = torch.randint(1, 1 << 16, (n_keys,), dtype=torch.int64, device="cuda")
        need = vr.cast_scratch_bytes(n, n_keys)
        scratch = zeros(need)
        by, out, go, wo = zeros(n, torch.int64), zeros(n, torch.int32), zeros(n, torch.int32), zeros(n, torch.int64)
        disp, count, found = zeros(2 * n, torch.int64), zeros(1, torch.int64), zeros(3, torch.int32)
        roll = zeros(n_keys, torch.int64)
        spread = torch.randperm(n_keys, device="cuda")[:n].to(torch.int32)
        revote = spread.clone()
        later = torch.arange(n // 2, n, 50, device="cuda")                       # 1 % of the ballots, in the second half
        revote[later] = spread[later - n // 2]
        for pattern, idx in (("spread", spread), ("revote", revote), ("flood", zeros(n, torch.int32))):
            for prior_name in ("empty", "full"):
                # full: every key counted a ballot of sequence number 5 before; the batch's numbers begin at 1000
                prior = zeros(n_keys, torch.int64) if prior_name == "empty" else torch.full((n_keys,), 6, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()

                def cast():
                    roll.copy_(prior)
                    vr.cast_device(n, idx.data_ptr(), 1000, roll.data_ptr(), n_keys, by.data_ptr(), found.data_ptr(), scratch.data_ptr(), need,
                                   d_roster_groups=groups.data_ptr(), d_roster_weights=weights.data_ptr(), d_status_out=out.data_ptr(),
                                   d_groups_out=go.data_ptr(), d_weights_out=wo.data_ptr(), d_displaced=disp.data_ptr(),
                                   d_displaced_count=count.data_ptr(), stream=stream)

                cast_ms = event_ms(cast)
                reset_ms = event_ms(lambda: roll.copy_(prior))
                cast()
                torch.cuda.synchronize()
                f_cast, displaced = found.cpu().tolist(), int(count.item())
                check_ms = event_ms(lambda: vr.check_device(n, idx.data_ptr(), 1000, roll.data_ptr(), n_keys, by.data_ptr(), found.data_ptr(),
                                                            d_roster_groups=groups.data_ptr(), d_roster_weights=weights.data_ptr(),
                                                            d_status_out=out.data_ptr(), d_groups_out=go.data_ptr(), d_weights_out=wo.data_ptr(),
                                                            stream=stream))
                f_check = found.cpu().tolist()
                voters = {"spread": n, "revote": n - len(later), "flood": 1}[pattern]
                assert f_cast == [n - voters, voters if prior_name == "full" else 0, 0] and displaced == f_cast[1], (pattern, prior_name, f_cast, displaced)
                assert f_check == [n - voters, 0, 0], (pattern, prior_name, f_check)
                sig_ms, verify_ms = beside[n]
                say(f"{n:8d} {n_keys:9d} {pattern:>7s} {prior_name:>6s} {cast_ms:8.3f} {reset_ms:7.3f} {n / max(cast_ms - reset_ms, 1e-3) / 1e3:9.1f} {check_ms:8.3f} "
                    f"{cast_ms / sig_ms:8.4f} {cast_ms / verify_ms:11.5f} {f_cast[0]:10d} {displaced:9d} {need / 1e6:10.1f}")
                if pattern == "flood":
                    flood_at[n] = max(flood_at.get(n, 0.0), cast_ms)
        del groups, weights, scratch, by, out, go, wo, disp, roll, spread, revote
        torch.cuda.empty_cache()

top = max(SIZES)
sig_ms = beside[top][0]
say(f"flood at n = {top}: the slowest flood cast takes {flood_at[top]:.3f} ms, the signature pass {sig_ms:.3f} ms over as many items "
    f"({flood_at[top] / sig_ms:.3f} of it): " + ("the pass IS the slowest link of the chain under a flood" if flood_at[top] > sig_ms
                                                else "the pass is not the slowest link of the chain under a flood"))
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
print(f"wrote {OUT}")
