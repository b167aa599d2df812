#!/usr/bin/env python3
"""Developer probe: what verifying a re-encryption shuffle costs (eg_shuffle_verify_device), beside the detour that the chain equation
would take through the entries the library had before: eg_vartime_multi_mul_batch_device(n = N, terms = 2) with the generator term,
plus a gather of (c^_i, c^_(i-1)) and a byte compare (torch).
Shuffles of N = 2^12, 2^16 and 2^20 rows are made by the model (tests/shuffle_ref.py) over the library's primitive tier; the last reaches
the bucket method inside the shuffle's products.  Every figure is HIP events around the call on the current stream, a warm-up call and
then REPS calls: the median, and the smallest and largest of them as the spread.  The verdict of every timed call must be 0.
One run: recorded, not gated.  The two-decode form of the chain kernel (tools/variants/shuffle_chain_two_decode.patch) is measured by
running the same probe on that build (EG_LIB=build_variants/libeg_two_decode.so, --tag two-decode); the stages of the pass have no entries
of their own, so their split comes from a kernel trace of this probe (--trace-size N runs one size without timing it).

Every size is a process of its own under a time limit; the first one that fails ends the probe.

  shuffle_probe.py [--sizes 4096,65536] [--tag NAME] [--out PATH]     appends to PATH (default profiles/r24_shuffle.txt)"""
import random
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SIZES, REPS, STEP_LIMIT_S = (1 << 12, 1 << 16, 1 << 20), 5, 900
HEAD = f"{'build':>11s} {'N':>8s} {'verify ms':>10s} {'min':>9s} {'max':>9s} {'detour ms':>10s} {'min':>9s} {'max':>9s} {'scratch MB':>11s} {'prove s':>8s}"


def step(n, tag, timed=True):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    import torch

    import elastic_elgamal_amd as eg
    import shuffle_ref as M

    ctx = eg.Context(0)
    maker = M.LibraryBackend(ctx)
    K = maker.mul_generator([0xC0FFEE])[0]
    prefix = b"probe/mixer-1"
    raw_key = eg.ShuffleVerifier.derive_key(ctx, b"probe key", n)
    key = [raw_key[32 * j:32 * j + 32] for j in range(n + 1)]
    t0 = time.time()
    case = M.make(maker, K, key, prefix, n, 24)
    prove_s = time.time() - t0
    v = eg.ShuffleVerifier(ctx, K, key=raw_key)
    need = v.verify_scratch_bytes(n)
    dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    d_in, d_out, d_key, d_proof = dev(b"".join(case["ins"])), dev(b"".join(case["outs"])), dev(raw_key), dev(case["proof"])
    d_verdict, d_found = torch.full((1,), 7, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def verify():
        v.verify_device(n, d_in.data_ptr(), d_out.data_ptr(), d_key.data_ptr(), d_proof.data_ptr(), d_verdict.data_ptr(), d_found.data_ptr(),
                        d_scratch.data_ptr(), need, prefix=prefix, stream=stream)

    def event_ms(fn, reps=REPS, warm=1):
        ts = []
        for k in range(warm + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if k >= warm:
                ts.append(a.elapsed_time(b))
        return statistics.median(ts), min(ts), max(ts)

    if not timed:
        verify()
        torch.cuda.synchronize()
        assert d_verdict.item() == 0
        return
    ver = event_ms(verify)
    assert d_verdict.item() == 0 and d_found.tolist()[:2] == [0, 0]
    # the detour: [-x]c^_i + [s'_i]c^_(i-1) + [s^_i]G through the product entry, gathered and compared with torch
    t, s, (c, chat, that, shat, sprime) = M.split_proof(n, case["proof"])
    seed1, _ = M.challenges_u(n, case["ins"], case["outs"], K, key, prefix, c)
    negx = dev(M.sc(-M.challenge_x(n, seed1, chat, that, t)))
    rows = d_proof[288:].view(5, n, 32)
    r = eg.Ristretto(ctx)
    msm_need = r.msm_scratch_bytes(n, 2)
    msm_scratch = torch.empty(max(msm_need, 16), dtype=torch.uint8, device="cuda")
    out, ok = torch.empty(n, 32, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    same = []

    def detour():
        prev = torch.cat([d_key[:32].view(1, 32), rows[1][:-1]])
        points = torch.stack([rows[1], prev], dim=1).contiguous()
        scalars = torch.stack([negx.view(1, 32).expand(n, 32), rows[4]], dim=1).contiguous()
        r.vartime_multi_mul_device(n, 2, scalars.data_ptr(), points.data_ptr(), out.data_ptr(), d_r=rows[3].data_ptr(),
                                   d_scratch=msm_scratch.data_ptr() if msm_need else 0, d_ok=ok.data_ptr(), stream=stream)
        same.append(torch.equal(out, rows[2]))

    det = event_ms(detour)
    assert all(same)
    print(f"ROW {tag:>11s} {n:8d} {ver[0]:10.3f} {ver[1]:9.3f} {ver[2]:9.3f} {det[0]:10.3f} {det[1]:9.3f} {det[2]:9.3f} {need / 1e6:11.1f} {prove_s:8.1f}", flush=True)
    print(f"DEVICE {ctx.name}", flush=True)


def main():
    args = sys.argv[1:]
    tag = args[args.index("--tag") + 1] if "--tag" in args else "product"
    if args[:1] == ["--step"]:
        return step(int(args[1]), tag)
    if "--trace-size" in args:
        return step(int(args[args.index("--trace-size") + 1]), tag, timed=False)
    out = Path(args[args.index("--out") + 1]) if "--out" in args else ROOT / "profiles" / "r24_shuffle.txt"
    sizes = [int(x) for x in args[args.index("--sizes") + 1].split(",")] if "--sizes" in args else SIZES
    rows, device = [], "?"
    for n in sizes:
        try:
            r = subprocess.run([sys.executable, __file__, "--step", str(n), "--tag", tag], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"N = {n}: no answer within {STEP_LIMIT_S} s; the probe ends here")
        if r.returncode != 0:
            sys.exit(f"N = {n}: exit status {r.returncode}; the probe ends here\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
        rows += [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        device = next((line[7:] for line in r.stdout.splitlines() if line.startswith("DEVICE ")), device)
        print(rows[-1], flush=True)
    new = not out.exists()
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as f:
        if new:
            f.write(f"device: {device}; a re-encryption shuffle of N rows made by tests/shuffle_ref.py; times in ms: median of {REPS} calls after a warm-up, "
                    "their smallest and largest; one run\n"
                    "verify: eg_shuffle_verify_device, the whole pass; detour: the chain equation alone as eg_vartime_multi_mul_batch_device(n = N, terms = 2) "
                    "+ generator term, with the gather and the byte compare in torch\n"
                    "build: product = the shipped library; two-decode = tools/variants/shuffle_chain_two_decode.patch; prove s: the model's prover (host time)\n"
                    + HEAD + "\n")
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
