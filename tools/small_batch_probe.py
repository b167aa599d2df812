#!/usr/bin/env python3
"""Developer probe: latency of small device-resident batches, the batch entry (eg_verify_*_batch_device) against the small-batch entry
(eg_verify_*_small_device), call + synchronize: single choice (5 options), multi-choice (3 of 16) and quadratic voting (5 options,
20 credits), and one wide ballot (single choice, 150 options).  Medians of 21 repetitions after 3 warm-up calls, what enqueueing a call
costs the host, the clock, whether both entries gave the same verdicts, and what one ballot costs one CPU core of the same box (the
oracle's verify, median of 21).  The batch entry alone is followed on to 16 384 and 65 536 ballots (the end of the flat part of its curve).

  small_batch_probe.py            the whole table
  small_batch_probe.py --brief    n = 1, 64 and 1 024 of the three main shapes only (A/B runs: EG_LIB=build_variants/libeg_NAME.so)"""
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import elastic_elgamal_amd as eg
from oracle import oracle as o

BRIEF = "--brief" in sys.argv[1:]
pk = bytes.fromhex("a6adb6e9c0ae8d54c26e6e56b5ccd7a16bb0e1951abe4d7ee7028e3d4eca8531")
o.lib()
ctx = eg.Context(0)
SIZES = (1, 64, 1024) if BRIEF else (1, 4, 16, 64, 256, 1024, 4096)
BATCH_ONLY = () if BRIEF else (16384, 65536)


def median_ms(fn, n, d, st, reps=21, warm=3):
    for _ in range(warm):
        fn(n, d.data_ptr(), st.data_ptr()); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(n, d.data_ptr(), st.data_ptr()); torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def enqueue_ms(fn, n, d, st, reps=20):
    """what the call costs the host when nobody waits for the result: reps calls back to back, one synchronize at the end"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(n, d.data_ptr(), st.data_ptr())
    dt = (time.perf_counter() - t0) / reps
    torch.cuda.synchronize()
    return dt * 1e3


def clock_mhz():
    try:
        _, mhz = ctx.selfbench_fmul(0.05)
        return mhz
    except Exception:
        return float("nan")


shapes = [("single choice, 5 options", lambda: eg.ChoiceParams(ctx, pk, 5, True), {}, SIZES, BATCH_ONLY),
          ("multi-choice, 3 of 16", lambda: eg.ChoiceParams(ctx, pk, 16, False), {"n_selected": 3}, SIZES, ()),
          ("quadratic voting, 5 options, 20 credits", lambda: eg.QuadraticVotingParams(ctx, pk, 5, 20), {}, SIZES, ())]
if not BRIEF:
    shapes.append(("single choice, 150 options", lambda: eg.ChoiceParams(ctx, pk, 150, True), {}, (1, 64), ()))
print(f"device: {ctx.name}; shader clock {clock_mhz():.0f} MHz; medians of 21 call + synchronize after 3 warm-up calls, device-resident ballots; "
      f"library {eg.library_path().name}")
for name, make, kw, sizes, batch_only in shapes:
    p = make()
    N = max(sizes + batch_only)
    d = torch.empty(N * p.ballot_size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(1, 0, N, d.data_ptr(), **kw)
    ctx.synchronize()
    if N > 7:
        d[7 * p.ballot_size + 40] ^= 1            # one rejected ballot among the first sixteen
    sa = torch.empty(N, dtype=torch.int32, device="cuda")
    sb = torch.empty(N, dtype=torch.int32, device="cuda")
    one = bytes(d[: p.ballot_size].cpu().numpy())
    op = o.QvParams(pk, 5, 20) if isinstance(p, eg.QuadraticVotingParams) else o.ChoiceParams(pk, p.n_options, p.single)
    cpu = []
    for _ in range(24):
        t0 = time.perf_counter()
        verdict = op.verify(one)
        cpu.append(time.perf_counter() - t0)
    assert verdict == 0
    print(f"{name} ({p.ballot_size} bytes per ballot); one ballot on one CPU core (oracle): {statistics.median(cpu[3:]) * 1e3:.3f} ms")
    print(f"  {'n':>5s} {'batch ms':>9s} {'small ms':>9s} {'small/batch':>11s} {'small us/ballot':>15s} {'enqueue batch':>13s} {'enqueue small':>13s}  verdicts")
    for n in sizes:
        tb = median_ms(p.verify_batch_device, n, d, sa)
        ts = median_ms(p.verify_small_device, n, d, sb)
        same = bool((sa[:n] == sb[:n]).all())
        eb = enqueue_ms(p.verify_batch_device, n, d, sa)
        es = enqueue_ms(p.verify_small_device, n, d, sb)
        print(f"  {n:5d} {tb:9.3f} {ts:9.3f} {ts / tb:11.2f} {ts * 1e3 / n:15.1f} {eb:13.3f} {es:13.3f}  {'agree' if same else 'DIFFER'} ({int((sb[:n] == 0).sum())} accepted)", flush=True)
    for n in batch_only:
        tb = median_ms(p.verify_batch_device, n, d, sa)
        eb = enqueue_ms(p.verify_batch_device, n, d, sa)
        print(f"  {n:5d} {tb:9.3f} {'-':>9s} {'-':>11s} {'-':>15s} {eb:13.3f} {'-':>13s}  batch entry alone: {n / tb / 1e3:.3f} M ballots/s ({int((sa[:n] == 0).sum())} accepted)", flush=True)
    p.close()
    del d, sa, sb
