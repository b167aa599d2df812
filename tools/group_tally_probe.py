#!/usr/bin/env python3
"""Developer probe: what the per-group tally (eg_choice_tally_grouped_device) costs beside the verification it follows.
Device-resident 5-option single-choice ballots, n = 2^20 and 2^16; n_groups = 1, 100, 10^4, 10^5 with uniform group ids, and one skewed
case (half of the ballots in one group, the rest spread over 10^4).  Time of the grouped pass alone (HIP events, median of 5 after a
warm-up call), beside the batch verify call of the same ballots in the same process.  For n = 2^20 and 10^4 groups also the only route
without the pass: ballots sorted by group, one eg_verify_choice_small_device call between tally_reset_async and tally_encode_device per
group (wall clock from the first call to the last synchronisation).  A first measurement: recorded, not gated.

  group_tally_probe.py            the whole table
  group_tally_probe.py --brief    without the per-group route (12 s of calls)"""
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

import elastic_elgamal_amd as eg

BRIEF = "--brief" in sys.argv[1:]
pk = bytes.fromhex("a6adb6e9c0ae8d54c26e6e56b5ccd7a16bb0e1951abe4d7ee7028e3d4eca8531")
ctx = eg.Context(0)
p = eg.ChoiceParams(ctx, pk, 5, True)
stream = torch.cuda.current_stream().cuda_stream


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


def groups_for(kind, n, n_groups, rng):
    if kind == "uniform":
        return rng.integers(0, n_groups, n, dtype=np.uint32)
    g = rng.integers(1, n_groups, n, dtype=np.uint32)
    g[rng.random(n) < 0.5] = 0
    return g


print(f"device: {ctx.name}; piece sizes S1 / S2 from group_tally_host.hpp; times in ms")
print(f"{'n':>8s} {'groups':>7s} {'ids':>8s} {'grouped':>9s} {'verify':>9s} {'verify/grouped':>14s} {'scratch MB':>10s}")
for n in (1 << 20, 1 << 16):
    d = torch.zeros(n * p.ballot_size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(4242, 0, n, d.data_ptr())
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    verify_ms = event_ms(lambda: p.verify_batch_device(n, d.data_ptr(), status.data_ptr(), stream=stream))
    assert int(status.abs().sum().item()) == 0
    rng = np.random.default_rng(n)
    for kind, n_groups in (("uniform", 1), ("uniform", 100), ("uniform", 10**4), ("uniform", 10**5), ("half in 0", 10**4)):
        ids = groups_for(kind, n, n_groups, rng)
        d_groups = torch.from_numpy(ids.view(np.int32)).cuda()
        scratch = torch.empty(p.tally_grouped_scratch_bytes(n, n_groups), dtype=torch.uint8, device="cuda")
        tallies = torch.zeros(n_groups * 320, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(n_groups, dtype=torch.int32, device="cuda")
        bad = torch.zeros(2, dtype=torch.int32, device="cuda")
        ms = event_ms(lambda: p.tally_grouped_device(n, d.data_ptr(), status.data_ptr(), d_groups.data_ptr(), n_groups, scratch.data_ptr(),
                                                     tallies.data_ptr(), bad.data_ptr(), d_counts=counts.data_ptr(), stream=stream))
        assert bad.cpu().tolist() == [0, 0] and int(counts.sum().item()) == n
        print(f"{n:8d} {n_groups:7d} {kind:>8s} {ms:9.3f} {verify_ms:9.3f} {verify_ms / ms:14.1f} {scratch.numel() / 1e6:10.1f}")
        if n == 1 << 20 and n_groups == 10**4 and kind == "uniform" and not BRIEF:
            # the route without the pass: sort by group, then one small verify call per group around tally_reset / tally_encode
            order = torch.argsort(d_groups.to(torch.int64), stable=True)
            sorted_d = d.view(n, p.ballot_size)[order].contiguous().view(-1)
            sizes = torch.bincount(d_groups.to(torch.int64), minlength=n_groups).cpu().tolist()
            assert max(sizes) <= eg.SMALL_BATCH_MAX
            per_group = torch.zeros(n_groups * 320, dtype=torch.uint8, device="cuda")
            route = torch.cuda.Stream().cuda_stream          # (a stream of its own: tally_reset on the null stream is the synchronous form)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lo = 0
            for g, m in enumerate(sizes):
                p.tally_reset(stream=route)
                p.verify_small_device(m, sorted_d.data_ptr() + lo * p.ballot_size, status.data_ptr() + 4 * lo, stream=route)
                p.tally_encode_device(per_group.data_ptr() + 320 * g, stream=route)
                lo += m
            torch.cuda.synchronize()
            route_s = time.perf_counter() - t0
            same = bool(torch.equal(per_group, tallies))
            print(f"         the same 10^4 tallies by one eg_verify_choice_small_device call per group (ballots pre-sorted): {route_s:.2f} s, "
                  f"tallies equal: {same}; batch verify + grouped pass: {(verify_ms + ms) / 1e3:.3f} s")
        del scratch, tallies
    p.tally_reset()
    del d
