#!/usr/bin/env python3
"""Developer probe: what the weighted per-group tally (eg_choice_tally_weighted_device) costs beside the unweighted grouped pass and the
verification it follows.  2^20 device-resident 5-option single-choice ballots; weight_bits 1 / 16 / 32 / 64, each with one group, 10^4
groups with uniform ids, and half of the ballots in one group (the rest spread over 10^4).  Time of the pass alone (HIP events, median of
5 after a warm-up call), beside the grouped pass over the same groups and the batch verify call of the same ballots in the same process.
For one group also the only route without the pass: gather the 10 strided wire items of every ballot into contiguous arrays, widen the
weights to 32-byte scalars, and one eg_vartime_multi_mul_batch_device call with one problem per tally slot.
Every run is sample-checked against the CPU oracle (oracle.point_multi_mul): slot 0 of the largest group and every slot of a small one,
and the weight sums against Python integers.  A first measurement: recorded, not gated."""
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

import elastic_elgamal_amd as eg
from oracle import oracle

pk = oracle.keypair_from_seed(12345)[1]
ctx = eg.Context(0)
p = eg.ChoiceParams(ctx, pk, 5, True)
grp = eg.Ristretto(ctx)
stream = torch.cuda.current_stream().cuda_stream
N, SIZE, SLOTS = 1 << 20, p.ballot_size, 10


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


def oracle_slot(view, members, weights, slot):
    """sum [w] x tally item `slot` over the ballots `members`, by the oracle"""
    pts = view[torch.from_numpy(members.astype(np.int64)).cuda(), 32 * slot:32 * slot + 32].contiguous().cpu().numpy().tobytes()
    sc = np.zeros((len(members), 4), dtype=np.uint64)
    sc[:, 0] = weights[members]
    return oracle.point_multi_mul(sc.tobytes(), pts)


d = torch.zeros(N * SIZE, dtype=torch.uint8, device="cuda")
p.encrypt_batch_device(4242, 0, N, d.data_ptr())
status = torch.zeros(N, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
verify_ms = event_ms(lambda: p.verify_batch_device(N, d.data_ptr(), status.data_ptr(), stream=stream))
assert int(status.abs().sum().item()) == 0
p.tally_reset()
view = d.view(N, SIZE)
rng = np.random.default_rng(13)
cases = {}
for name, n_groups in (("one group", 1), ("10^4 uniform", 10**4), ("half in 0", 10**4)):
    ids = rng.integers(0 if name != "half in 0" else 1, n_groups, N, dtype=np.uint32) if n_groups > 1 else np.zeros(N, dtype=np.uint32)
    if name == "half in 0":
        ids[rng.random(N) < 0.5] = 0
    cases[name] = (n_groups, ids)

print(f"device: {ctx.name}; n = 2^20 five-option ballots, all accepted; batch verify call {verify_ms:.1f} ms; times in ms")
print(f"{'groups':>13s} {'bits':>5s} {'weighted':>9s} {'grouped':>9s} {'weighted/grouped':>16s} {'verify/weighted':>15s} {'scratch MB':>10s}  oracle sample")
for name, (n_groups, ids) in cases.items():
    d_groups = torch.from_numpy(ids.view(np.int32)).cuda()
    tallies = torch.zeros(n_groups * 320, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n_groups, dtype=torch.int32, device="cuda")
    sums = torch.zeros((n_groups, 2), dtype=torch.int64, device="cuda")
    bad = torch.zeros(3, dtype=torch.int32, device="cuda")
    g_scratch = torch.empty(p.tally_grouped_scratch_bytes(N, n_groups), dtype=torch.uint8, device="cuda")
    grouped_ms = event_ms(lambda: p.tally_grouped_device(N, d.data_ptr(), status.data_ptr(), d_groups.data_ptr(), n_groups, g_scratch.data_ptr(),
                                                         tallies.data_ptr(), bad.data_ptr(), d_counts=counts.data_ptr(), stream=stream))
    assert bad.cpu().tolist()[:2] == [0, 0]
    del g_scratch
    scratch = torch.empty(p.tally_weighted_scratch_bytes(N, n_groups), dtype=torch.uint8, device="cuda")
    small = n_groups - 1
    for bits in (1, 16, 32, 64):
        weights = rng.integers(0, (1 << bits) - 1, N, dtype=np.uint64, endpoint=True)
        d_weights = torch.from_numpy(weights.view(np.int64)).cuda()
        ms = event_ms(lambda: p.tally_weighted_device(N, d.data_ptr(), status.data_ptr(), d_weights.data_ptr(), bits,
                                                      d_groups.data_ptr() if n_groups > 1 else 0, n_groups, scratch.data_ptr(), tallies.data_ptr(),
                                                      bad.data_ptr(), d_weight_sums=sums.data_ptr(), d_counts=counts.data_ptr(), stream=stream))
        assert bad.cpu().tolist() == [0, 0, 0] and int(counts.sum().item()) == N
        got = tallies.view(n_groups, 320).cpu().numpy()
        words = sums.cpu().numpy().view(np.uint64).tolist()
        checked = []
        for g, slots in ((0, (0,)), (small, range(SLOTS))) if n_groups > 1 else ((0, (0,)),):
            members = np.nonzero(ids == g)[0]
            assert words[g][0] | (words[g][1] << 64) == sum(int(w) for w in weights[members])
            for t in slots:
                assert bytes(got[g, 32 * t:32 * t + 32]) == oracle_slot(view, members, weights, t), (name, bits, g, t)
            checked.append(f"group {g}: {len(members)} ballots x {len(slots)} slot(s)")
        print(f"{name:>13s} {bits:5d} {ms:9.3f} {grouped_ms:9.3f} {ms / grouped_ms:16.2f} {verify_ms / ms:15.1f} {scratch.numel() / 1e6:10.1f}  ok ({'; '.join(checked)})")
        if n_groups == 1:
            # the route without the pass: contiguous copies of the ten wire items and of the weights as 32-byte scalars, one problem per slot
            msm_scratch = torch.empty(max(grp.msm_scratch_bytes(SLOTS, N), 16), dtype=torch.uint8, device="cuda")
            out = torch.zeros(SLOTS * 32, dtype=torch.uint8, device="cuda")

            def detour():
                pts = view[:, :32 * SLOTS].reshape(N, SLOTS, 32).permute(1, 0, 2).contiguous()
                sc = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
                sc[:, 0] = d_weights
                scs = sc.view(torch.uint8).reshape(1, N, 32).expand(SLOTS, N, 32).contiguous()
                grp.vartime_multi_mul_device(SLOTS, N, scs.data_ptr(), pts.data_ptr(), out.data_ptr(), 0, msm_scratch.data_ptr(), stream=stream)
                return pts, scs

            try:
                detour_ms = event_ms(detour, reps=3)
            except eg.EgError as e:
                print(f"{'':>13s} {'':>5s} gather + eg_vartime_multi_mul_batch_device refused: {e}")
                continue
            same = bytes(out.cpu().numpy()) == bytes(got[0])
            print(f"{'':>13s} {'':>5s} the same totals by gather + eg_vartime_multi_mul_batch_device (10 problems of 2^20 terms): {detour_ms:9.3f} ms, "
                  f"equal: {same}, scratch {msm_scratch.numel() / 1e6:.0f} MB + {2 * SLOTS * N * 32 / 1e6:.0f} MB of copies")
            del msm_scratch
    del scratch, tallies
