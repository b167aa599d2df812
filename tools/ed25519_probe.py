#!/usr/bin/env python3
"""Developer probe: what the Ed25519 signature pass (eg_ed25519_verify_device) costs beside the ballot verification it precedes.
Device-resident items, n = 2^16 and 2^20: five-option single-choice ballots (736 B), 3-of-16 multi-choice ballots (2080 B) of the GPU
generator, and 32-byte random messages; every item signed on the GPU under a key of its own, prefix of 11 bytes.  Per row (HIP events,
median of 5 after a warm-up call):
  sig       the pass                                   -> signatures / s
  hash      eg_sha512_batch_device over R || A-sized prefix + the same messages (the hashing's share of the pass)
  dmul      eg_vartime_multi_mul_batch_device, one term plus the generator term, over n (scalar, point, scalar) operands in the same
            process: the double-base product the pass is built around
  verify    eg_verify_choice_batch_device over the same ballots in the same process (ballot rows only)
  sign      the signer (eg_ed25519_sign_batch_device)  -> signatures / s
A first measurement, one run: recorded, not gated.

  ed25519_probe.py               writes profiles/r17_ed25519.txt
  ed25519_probe.py --out PATH    writes PATH"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

import elastic_elgamal_amd as eg

args = sys.argv[1:]
OUT = Path(args[args.index("--out") + 1]) if "--out" in args else ROOT / "profiles" / "r17_ed25519.txt"
SIZES = [int(a) for a in args[args.index("--sizes") + 1].split(",")] if "--sizes" in args else [1 << 16, 1 << 20]
pk = bytes.fromhex("a6adb6e9c0ae8d54c26e6e56b5ccd7a16bb0e1951abe4d7ee7028e3d4eca8531")
ctx = eg.Context(0)
ed, group = eg.Ed25519(ctx), eg.Ristretto(ctx)
stream = torch.cuda.current_stream().cuda_stream
PREFIX = b"election-42"
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


say(f"device: {ctx.name}; prefix of {len(PREFIX)} bytes; times in ms, one run")
say(f"{'items':>12s} {'bytes':>6s} {'n':>8s} {'sig':>9s} {'Msig/s':>7s} {'hash':>8s} {'hash/sig':>8s} {'dmul':>8s} {'sig/dmul':>8s} {'verify':>10s} {'sig/verify':>10s} "
    f"{'sign':>9s} {'Msign/s':>7s} {'scratch MB':>10s}")
d_prefix = torch.frombuffer(bytearray(PREFIX), dtype=torch.uint8).cuda()
shapes = (("single-5", eg.ChoiceParams(ctx, pk, 5, True), 0), ("multi-3of16", eg.ChoiceParams(ctx, pk, 16, False), 3), ("random-32", None, 0))
for name, params, n_selected in shapes:
    size = params.ballot_size if params else 32
    for n in SIZES:
        if params:
            msgs = zeros(n * size)
            if n_selected:
                params.encrypt_batch_device(4242, 0, n, msgs.data_ptr(), n_selected=n_selected)
            else:
                params.encrypt_batch_device(4242, 0, n, msgs.data_ptr())
        else:
            msgs = torch.randint(0, 256, (n * size,), dtype=torch.uint8, device="cuda")
        seeds = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device="cuda")
        keys, sigs, digests = zeros(32 * n), zeros(64 * n), zeros(64 * n)
        status, ballot_status = torch.full((n,), 7, dtype=torch.int32, device="cuda"), zeros(n, torch.int32)
        need = ed.verify_scratch_bytes(n)
        scratch = zeros(need)
        torch.cuda.synchronize()
        ed.keypairs_device(n, seeds.data_ptr(), keys.data_ptr(), stream=stream)
        sign_ms = event_ms(lambda: ed.sign_device(n, seeds.data_ptr(), msgs.data_ptr(), size, size, sigs.data_ptr(), d_prefix.data_ptr(), len(PREFIX),
                                                  stream=stream), reps=3)
        sig_ms = event_ms(lambda: ed.verify_device(n, msgs.data_ptr(), size, size, keys.data_ptr(), n, sigs.data_ptr(), status.data_ptr(),
                                                   scratch.data_ptr(), need, prefix=PREFIX, stream=stream))
        assert int(status.abs().sum().item()) == 0, "a signature of the GPU signer was refused"
        # the hash of the pass reads 64 + prefix + size bytes an item: the same number of blocks with a prefix 64 bytes longer
        d_long = torch.frombuffer(bytearray(bytes(64) + PREFIX), dtype=torch.uint8).cuda()
        hash_ms = event_ms(lambda: ed.sha512_device(n, msgs.data_ptr(), size, size, digests.data_ptr(), d_long.data_ptr(), 64 + len(PREFIX), stream=stream))
        # double-base products over n operands: scalars = the S halves (canonical), points = [S]G as ristretto255 encodings
        scalars = sigs.view(n, 64)[:, 32:].contiguous()
        points, out, ok = zeros(32 * n), zeros(32 * n), zeros(n)
        group.vartime_multi_mul_device(n, 0, 0, 0, points.data_ptr(), d_r=scalars.data_ptr(), stream=stream)
        dmul_ms = event_ms(lambda: group.vartime_multi_mul_device(n, 1, scalars.data_ptr(), points.data_ptr(), out.data_ptr(), d_r=scalars.data_ptr(),
                                                                  d_ok=ok.data_ptr(), stream=stream))
        assert int(ok.sum().item()) == n
        if params:
            verify_ms = event_ms(lambda: params.verify_batch_device(n, msgs.data_ptr(), ballot_status.data_ptr(), stream=stream), reps=3)
            assert int(ballot_status.abs().sum().item()) == 0
            params.tally_reset()
            vcol, rcol = f"{verify_ms:10.3f}", f"{sig_ms / verify_ms:10.4f}"
        else:
            vcol, rcol = f"{'-':>10s}", f"{'-':>10s}"
        say(f"{name:>12s} {size:6d} {n:8d} {sig_ms:9.3f} {n / sig_ms / 1e3:7.2f} {hash_ms:8.3f} {hash_ms / sig_ms:8.3f} {dmul_ms:8.3f} {sig_ms / dmul_ms:8.2f} "
            f"{vcol} {rcol} {sign_ms:9.3f} {n / sign_ms / 1e3:7.2f} {need / 1e6:10.1f}")
        del msgs, seeds, keys, sigs, digests, scratch, points, out
        torch.cuda.empty_cache()

OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
print(f"wrote {OUT}")
