#!/usr/bin/env python3
"""Developer probe: what a batch costs with the board's table kept between batches (eg_choice_weed_indexed_device) and with the table
rebuilt in every call (eg_choice_weed_device), in the same process over the same board.
Device-resident 5-option single-choice ballots of the GPU generator, n = 2^16 and 2^20, no duplicates, beside boards of 0, 5 x 10^6 and
5 x 10^7 ciphertexts (random bytes: no hits).  Both passes with the append (HIP events, median of 5 after a warm-up call; the index is
rebuilt, untimed, in front of every round so that each starts from an index over exactly the board), their scratch, the build of the
index alone, a find of 2^20 keys (half of them on the board where it has that many) and the batch verify call of the same ballots.
One run: recorded, not gated.

Every configuration is a process of its own under a time limit; the first one that fails ends the probe.

  weed_index_probe.py               writes profiles/r23_weed_index.txt
  weed_index_probe.py --out PATH    writes PATH"""
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BATCHES, BOARDS, STEP_LIMIT_S = (1 << 16, 1 << 20), (0, 5_000_000, 50_000_000), 240
HEAD = (f"{'n':>8s} {'board':>9s} {'indexed':>9s} {'stateless':>10s} {'ratio':>6s} {'scratch MB':>11s} {'(stateless)':>12s} {'index MB':>9s} "
        f"{'build':>9s} {'find 2^20':>10s} {'verify':>9s}")


def step(n, n_prior):
    sys.path.insert(0, str(ROOT))
    import torch

    import elastic_elgamal_amd as eg

    pk = bytes.fromhex("a6adb6e9c0ae8d54c26e6e56b5ccd7a16bb0e1951abe4d7ee7028e3d4eca8531")
    ctx = eg.Context(0)
    p = eg.ChoiceParams(ctx, pk, 5, True)
    K, size, seed = 5, p.ballot_size, 0x5EED0FACADE
    stream = torch.cuda.current_stream().cuda_stream

    def event_ms(fn, reps=5, warm=1, prepare=None):
        ts = []
        for k in range(warm + reps):
            if prepare:
                prepare()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if k >= warm:
                ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    d = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
    p.encrypt_batch_device(4242, 0, n, d.data_ptr())
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    verify_ms = event_ms(lambda: p.verify_batch_device(n, d.data_ptr(), status.data_ptr(), stream=stream), reps=3)
    assert int(status.abs().sum().item()) == 0
    cap = n_prior + n * K
    board = torch.empty(cap * 64, dtype=torch.uint8, device="cuda")
    if n_prior:
        board[: n_prior * 64] = torch.randint(0, 256, (n_prior * 64,), dtype=torch.uint8, device="cuda")
    index = torch.empty(ctx.weed_index_bytes(cap), dtype=torch.uint8, device="cuda")
    over = torch.zeros(1, dtype=torch.int32, device="cuda")

    def build():
        ctx.weed_index_build_device(n_prior, board.data_ptr(), cap, seed, index.data_ptr(), over.data_ptr(), stream=stream)

    build_ms = event_ms(build)
    assert over.item() == 0
    n_q, on_board = 1 << 20, min(n_prior, 1 << 19)
    queries = torch.randint(0, 256, (n_q * 64,), dtype=torch.uint8, device="cuda")
    queries[: on_board * 64] = board[: on_board * 64]
    pos = torch.zeros(n_q, dtype=torch.int32, device="cuda")
    find_ms = event_ms(lambda: ctx.weed_index_find_device(n_q, queries.data_ptr(), n_prior, board.data_ptr(), cap, index.data_ptr(), seed,
                                                          pos.data_ptr(), stream=stream))
    assert pos[:on_board].tolist() == list(range(on_board)) and int((pos[on_board:] != -1).sum().item()) == 0
    need_s, need_i = p.weed_scratch_bytes(n, n_prior), p.weed_indexed_scratch_bytes(n)
    big, small = torch.empty(need_s, dtype=torch.uint8, device="cuda"), torch.empty(need_i, dtype=torch.uint8, device="cuda")
    dups = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    founds = [torch.zeros(3, dtype=torch.int32, device="cuda") for _ in range(2)]
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    stateless_ms = event_ms(lambda: p.weed_device(n, d.data_ptr(), status.data_ptr(), n_prior, board.data_ptr(), cap, 77, big.data_ptr(),
                                                  dups[0].data_ptr(), founds[0].data_ptr(), d_board_count=count.data_ptr(), stream=stream))

    def prepare():
        build()
        torch.cuda.synchronize()

    indexed_ms = event_ms(lambda: p.weed_indexed_device(n, d.data_ptr(), status.data_ptr(), n_prior, board.data_ptr(), cap, index.data_ptr(), seed,
                                                        78, small.data_ptr(), dups[1].data_ptr(), founds[1].data_ptr(),
                                                        d_board_count=count[1:].data_ptr(), stream=stream), prepare=prepare)
    assert founds[0].tolist() == founds[1].tolist() == [0, 0, 0] and count.tolist() == [cap, cap] and torch.equal(dups[0], dups[1])
    p.tally_reset()
    print(f"ROW {n:8d} {n_prior:9d} {indexed_ms:9.3f} {stateless_ms:10.3f} {stateless_ms / indexed_ms:6.1f} {need_i / 1e6:11.1f} {need_s / 1e6:12.1f} "
          f"{index.numel() / 1e6:9.1f} {build_ms:9.3f} {find_ms:10.3f} {verify_ms:9.3f}", flush=True)
    print(f"DEVICE {ctx.name}", flush=True)


def main():
    args = sys.argv[1:]
    if args[:1] == ["--step"]:
        return step(int(args[1]), int(args[2]))
    out = Path(args[args.index("--out") + 1]) if "--out" in args else ROOT / "profiles" / "r23_weed_index.txt"
    rows, device = [], "?"
    for n in BATCHES:
        for n_prior in BOARDS:
            try:
                r = subprocess.run([sys.executable, __file__, "--step", str(n), str(n_prior)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
            except subprocess.TimeoutExpired:
                sys.exit(f"n = {n}, board = {n_prior}: no answer within {STEP_LIMIT_S} s; the probe ends here")
            if r.returncode != 0:
                sys.exit(f"n = {n}, board = {n_prior}: exit status {r.returncode}; the probe ends here\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
            rows += [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
            device = next((line[7:] for line in r.stdout.splitlines() if line.startswith("DEVICE ")), device)
            print(rows[-1], flush=True)
    lines = [f"device: {device}; 5-option single-choice ballots, 5 keys of 64 bytes each, no duplicates; times in ms, one run",
             "indexed / stateless: eg_choice_weed_indexed_device / eg_choice_weed_device with the append, same process, same board; ratio = stateless / indexed",
             "build: eg_weed_index_build_device over the whole board; find: eg_weed_index_find_device of 2^20 keys; verify: the batch verify call",
             HEAD, *rows]
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
