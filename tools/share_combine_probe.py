#!/usr/bin/env python3
"""Developer probe: what the batched share combination (eg_combine_shares_batch_device) costs, and beside what.
m = 5, 256, 50 000 and 2^20 device-resident ciphertexts (the tally items of generated ballots under a Shamir key) at 2-of-3, 7-of-10 and
33-of-64, shares made by eg_share_prove_batch_device and checked by eg_verify_proof_batch_device.  Per row:
  pass      the whole entry (HIP events on the stream, median of 5 after a warm-up call)
  stages    k_sc_select / k_sc_coeffs / k_sc_combine of one call, from the kernel records of torch's profiler (n/a where it gives none)
  select    the entry with one column too few: the walk alone, nothing to combine
  calls     the route of the parent commit, eg_combine_shares + eg_point_add_batch per ciphertext (m <= 256: it runs for seconds beyond)
  detour    replicated coefficients, the chosen dh gathered problem-major and one eg_vartime_multi_mul_batch_device call (B - D not included)
Then, at m = 50 000, key sets of 1, 8, 9, 16 and 17 shares: k_sc_coeffs at one share is the lane's inversion almost alone, and the steps
8 -> 9 and 16 -> 17 add a chain of 252 doublings where the steps between them add a term - the two prices that decide the chunk size.
Every run is sample-checked against the CPU oracle ([x]R by oracle.point_multi_mul).  A first measurement: recorded, not gated.
usage: share_combine_probe.py [output file, default profiles/r14_share_combine.txt]"""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch

import elastic_elgamal_amd as eg
import share_combine_ref as R
from elastic_elgamal_amd import tally as T
from oracle import oracle

OUT = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "r14_share_combine.txt"
ctx = eg.Context(0)
grp = eg.Ristretto(ctx)
stream = torch.cuda.current_stream().cuda_stream
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)
    OUT.write_text("\n".join(lines) + "\n")


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


def stage_ms(fn):
    """device time of the three kernels of one call, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        got = {}
        for e in prof.events():
            for name in ("k_sc_select", "k_sc_coeffs", "k_sc_combine"):
                if name in e.name:
                    us = e.device_time if hasattr(e, "device_time") else e.cuda_time
                    got[name] = got.get(name, 0.0) + us / 1e3
        return got if len(got) == 3 else None
    except Exception:          # noqa: BLE001
        return None


class Setup:
    """m ciphertexts under a shares_n-key set and t columns of verified shares, all in device memory"""

    def __init__(self, shares_n, threshold, m, seed=1):
        self.shares, self.t, self.m = shares_n, threshold, m
        self.ks = R.KeySet(oracle, shares_n, threshold, seed)
        p = eg.ChoiceParams(ctx, self.ks.shared_key, 5, True)
        n_ballots = (m + 4) // 5
        wire = torch.zeros(n_ballots * p.ballot_size, dtype=torch.uint8, device="cuda")
        p.encrypt_batch_device(4242, 0, n_ballots, wire.data_ptr())
        ctx.synchronize()
        self.cts = wire.view(n_ballots, p.ballot_size)[:, :320].reshape(-1, 64)[:m].contiguous()
        rs = self.cts[:, :32].contiguous()
        self.indexes = list(range(shares_n - threshold, shares_n))          # the last t participants: the largest index differences
        self.items = torch.zeros((threshold, m, 128), dtype=torch.uint8, device="cuda")
        self.status = torch.full((threshold, m), -1, dtype=torch.int32, device="cuda")
        ok = torch.zeros(m, dtype=torch.uint8, device="cuda")
        for j, i in enumerate(self.indexes):
            ver = eg.DecryptionShareVerifier(ctx, self.ks.shared_key, shares_n, threshold, i, self.ks.part_keys[i])
            ver.prove_device(R.sc(self.ks.sks[i]), 1000 * j, 0, m, rs.data_ptr(), self.items[j].data_ptr(), ok.data_ptr())
            ver.verify_device(m, self.items[j].data_ptr(), self.status[j].data_ptr())
            ctx.synchronize()
            ver.close()
        assert int(self.status.abs().sum().item()) == 0
        p.close()
        self.scratch = torch.empty(max(T.combine_shares_batch_scratch_bytes(threshold, m), 16), dtype=torch.uint8, device="cuda")
        self.dh = torch.zeros((m, 32), dtype=torch.uint8, device="cuda")
        self.plain = torch.zeros((m, 32), dtype=torch.uint8, device="cuda")
        self.combined = torch.zeros(m, dtype=torch.uint8, device="cuda")
        self.used = torch.zeros(m, dtype=torch.int64, device="cuda")
        self.bad = torch.zeros(4, dtype=torch.int32, device="cuda")

    def run(self, k=None):
        k = self.t if k is None else k
        T.combine_shares_batch_device(grp, self.shares, self.t, self.m, self.cts.data_ptr(), self.indexes[:k], self.items.data_ptr(),
                                      self.status.data_ptr(), self.combined.data_ptr(), self.bad.data_ptr(), self.scratch.data_ptr(),
                                      d_dh=self.dh.data_ptr(), d_plain=self.plain.data_ptr(), d_used=self.used.data_ptr(), stream=stream)

    def check(self):
        self.run()
        torch.cuda.synchronize()
        assert self.bad.cpu().tolist()[:3] == [0, 0, 0] and int(self.combined.sum().item()) == self.m
        for c in sorted({0, self.m // 2, self.m - 1}):
            want = oracle.point_multi_mul(R.sc(self.ks.secret), bytes(self.cts[c, :32].cpu().numpy()))
            assert bytes(self.dh[c].cpu().numpy()) == want, c
        return bytes(self.dh.cpu().numpy())

    def calls_ms(self):
        """eg_combine_shares + eg_point_add_batch per ciphertext, host buffers as that route has them"""
        cts = self.cts.cpu().numpy()
        items = self.items.cpu().numpy()
        shares = [[(i, bytes(items[j, c, 32:64])) for j, i in enumerate(self.indexes)] for c in range(self.m)]
        blinded = [bytes(cts[c, 32:]) for c in range(self.m)]

        def go():
            out = []
            for c in range(self.m):
                d = T.combine_shares(grp, self.t, shares[c], n_shares=self.shares)
                out.append((d, grp.element_add(blinded[c], d, subtract=True)[0]))
            return out

        go()
        t0 = time.perf_counter()
        out = go()
        ms = 1e3 * (time.perf_counter() - t0)
        assert b"".join(d for d, _ in out) == bytes(self.dh.cpu().numpy()) and b"".join(e for _, e in out) == bytes(self.plain.cpu().numpy())
        return ms

    def detour_ms(self):
        coef = np.frombuffer(b"".join(R.scaled_coefficients(oracle, self.indexes)), dtype=np.uint8).reshape(1, self.t, 32)
        d_coef = torch.from_numpy(coef.copy()).cuda()
        need = grp.msm_scratch_bytes(self.m, self.t)
        scratch = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        out = torch.zeros((self.m, 32), dtype=torch.uint8, device="cuda")

        def go():
            scalars = d_coef.expand(self.m, self.t, 32).contiguous()
            points = self.items[:, :, 32:64].permute(1, 0, 2).contiguous()
            grp.vartime_multi_mul_device(self.m, self.t, scalars.data_ptr(), points.data_ptr(), out.data_ptr(), 0, scratch.data_ptr() if need else 0,
                                         stream=stream)
            return scalars, points

        ms = event_ms(go, reps=3)
        torch.cuda.synchronize()
        assert bytes(out.cpu().numpy()) == bytes(self.dh.cpu().numpy())
        return ms, (need + 2 * self.m * self.t * 32) / 1e6


say(f"device: {ctx.name}; eg_combine_shares_batch_device over device-resident ciphertexts and verified shares, k = threshold columns; times in ms")
say(f"{'key set':>9s} {'m':>8s} {'pass':>9s} {'us/ct':>8s} {'select':>8s} {'coeffs':>8s} {'combine':>8s} {'one column short':>16s} {'calls':>10s} {'calls/pass':>10s} "
    f"{'detour':>9s} {'detour MB':>9s} {'scratch MB':>10s}")
for threshold, shares_n in ((2, 3), (7, 10), (33, 64)):
    for m in (5, 256, 50000, 1 << 20):
        s = Setup(shares_n, threshold, m)
        s.check()
        ms = event_ms(s.run)
        st = stage_ms(s.run)
        short = event_ms(lambda: s.run(threshold - 1))
        s.check()
        calls = s.calls_ms() if m <= 256 else None
        detour, detour_mb = s.detour_ms()
        stages = f"{st['k_sc_select']:8.3f} {st['k_sc_coeffs']:8.3f} {st['k_sc_combine']:8.3f}" if st else f"{'n/a':>8s} {'n/a':>8s} {'n/a':>8s}"
        say(f"{threshold:>4d}of{shares_n:<3d} {m:8d} {ms:9.3f} {1e3 * ms / m:8.3f} {stages} {short:16.3f} "
            + (f"{calls:10.1f} {calls / ms:10.1f}" if calls is not None else f"{'-':>10s} {'-':>10s}")
            + f" {detour:9.3f} {detour_mb:9.1f} {s.scratch.numel() / 1e6:10.1f}")
        del s
        torch.cuda.empty_cache()
say()
say("m = 50000, shares on both sides of the chunk seams (k_sc_coeffs at one share: the inversion and three products):")
say(f"{'key set':>9s} {'pass':>9s} {'select':>8s} {'coeffs':>8s} {'combine':>8s}")
for threshold in (1, 7, 8, 9, 16, 17):
    s = Setup(threshold, threshold, 50000)
    s.check()
    ms = event_ms(s.run)
    st = stage_ms(s.run)
    stages = f"{st['k_sc_select']:8.3f} {st['k_sc_coeffs']:8.3f} {st['k_sc_combine']:8.3f}" if st else f"{'n/a':>8s} {'n/a':>8s} {'n/a':>8s}"
    say(f"{threshold:>4d}of{threshold:<3d} {ms:9.3f} {stages}")
    del s
    torch.cuda.empty_cache()
