#!/usr/bin/env python3
"""Developer probe (not the benchmark): first measurement of the bounded discrete-log solver (eg_dlog_solver_*), recorded and not gated.
In ONE process: build time and table bytes at baby_bits 16 / 20 / 24 / 26 / 28; solve time for 5, 16 and 4000 elements in spans of
2^24, 2^32, 2^40 and 2^48 with the default solver - once with every value inside the span (a tally) and once with none (the whole span
is walked for every element: the worst case, and the one that gives giant steps per second); and the parent's way, eg_dlog_table_create
over 2^20 and 2^24 values plus eg_dlog_table_get.  Host-inclusive wall times (the calls are synchronous), medians of 3 after a warm-up (one run where a call takes seconds).
Writes profiles/r11_dlog_solver.txt, with the constants of csrc/dlog_host.hpp that were chosen from it.
usage: dlog_probe.py [output file]"""
import ctypes as C
import re
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import elastic_elgamal_amd as eg
from elastic_elgamal_amd import tally as T

L = 2**252 + 27742317777372353535851937790883648493
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "r11_dlog_solver.txt"
host = (ROOT / "elastic_elgamal_amd" / "csrc" / "dlog_host.hpp").read_text()
const = lambda name: int(re.search(name + r" = 1ull << (\d+)", host).group(1))
LAUNCH_LANES, CALL_STEPS = const("LAUNCH_LANES"), const("CALL_STEPS")
ctx = eg.Context(0)
grp = eg.Ristretto(ctx)
lines = [f"# tools/dlog_probe.py   [{ctx.name}]   first measurement: recorded, not gated",
         "# wall time of the synchronous host calls, medians of 3 after a warm-up, one process"]


def sc(x):
    return (x % L).to_bytes(32, "little")


def multiples(values):
    raw = grp.mul_generator(b"".join(sc(v) for v in values))
    return [raw[32 * i : 32 * i + 32] for i in range(len(values))]


def median3(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return sorted(ts)[len(ts) // 2]


lines.append("\n[build]  baby_bits  table_bytes  create_ms  solve_ms(16 elements, span 2^40, none inside)  giant_steps_per_s")
lo = 1_000_003
outside16 = None
build_ms = {}
for bits in (16, 20, 24, 26, 28):
    t = time.perf_counter()
    s = T.DiscreteLogSolver(grp, bits)
    dt = time.perf_counter() - t
    hi = lo + 2**40
    if outside16 is None:
        outside16 = multiples([hi + 1 + k for k in range(16)])
    assert s.solve(multiples([lo, hi - 1]), lo, hi) == [lo, hi - 1]
    ts = median3(lambda: s.solve(outside16, lo, hi))
    steps = 16 * (2**40 >> bits)
    lines.append(f"build {bits:2d} {s.table_bytes:12d} {dt * 1e3:10.1f} {ts * 1e3:10.2f} {steps / ts:.3e}")
    build_ms[bits] = dt * 1e3
    s.close()

s = T.DiscreteLogSolver(grp)
bits = (s.table_bytes // 16).bit_length() - 1
lines.append(f"\n[solve]  default solver, baby_bits {bits}:  n  log2(span)  inside_ms  none_inside_ms  giant_steps(none inside)  giant_steps_per_s")
best_rate, worst_16_48 = 0.0, None
for n in (5, 16, 4000):
    for ls in (24, 32, 40, 48):
        span = 1 << ls
        hi = lo + span
        if span > s.max_span(n):
            lines.append(f"solve {n:5d} {ls:2d}  refused: above max_span({n}) = {s.max_span(n)}")
            continue
        inside = [lo + (k * (span - 1)) // max(n - 1, 1) for k in range(n)]
        e_in, e_out = multiples(inside), multiples([hi + 1 + k for k in range(n)])
        steps = n * (((span - 1) >> bits) + 1)
        reps = 3 if steps < 1 << 33 else 1            # the widest calls take seconds: one timed run after the warm-up
        assert s.solve(e_in, lo, hi) == inside
        t_in = median3(lambda: s.solve(e_in, lo, hi), reps)
        assert s.solve(e_out, lo, hi) == [None] * n
        t_out = median3(lambda: s.solve(e_out, lo, hi), reps)
        if (n, ls) == (16, 48):
            worst_16_48 = t_out
        rate = steps / t_out
        if steps >= 1 << 26:
            best_rate = max(best_rate, rate)
        lines.append(f"solve {n:5d} {ls:2d} {t_in * 1e3:10.3f} {t_out * 1e3:10.3f} {steps:12d} {rate:.3e}")

lines.append("\n[parent]  eg_dlog_table_create over 1..=V, then eg_dlog_table_get of 16 elements:  log2(V)  create_ms  get_ms")
lib = eg._load()
for lv in (20, 24):
    V = 1 << lv
    arr = (C.c_uint64 * V)(*range(1, V + 1))
    h = C.c_void_p()
    t = time.perf_counter()
    eg._check(lib.eg_dlog_table_create(ctx._h, V, arr, C.byref(h)))
    t_create = time.perf_counter() - t
    vals = [1 + (k * (V - 1)) // 15 for k in range(16)]
    el = b"".join(multiples(vals))
    v, f = (C.c_uint64 * 16)(), C.create_string_buffer(16)
    t = time.perf_counter()
    eg._check(lib.eg_dlog_table_get(h, 16, el, v, f))
    t_get = time.perf_counter() - t
    assert list(v) == vals and f.raw == b"\1" * 16
    lib.eg_dlog_table_destroy(h)
    lines.append(f"parent {lv} {t_create * 1e3:10.1f} {t_get * 1e3:10.3f}")
    del arr

# the comparison that tests/test_gpu_dlog_solver.py asserts: medians of 5 after a warm-up
lo24, hi24 = 1, 1 + 2**24
vals24 = [lo24 + (k * (2**24 - 1)) // 15 for k in range(16)]
el24 = multiples(vals24)
arr20 = (C.c_uint64 * 2**20)(*range(1, 2**20 + 1))


def create20():
    h = C.c_void_p()
    eg._check(lib.eg_dlog_table_create(ctx._h, 2**20, arr20, C.byref(h)))
    lib.eg_dlog_table_destroy(h)


assert s.solve(el24, lo24, hi24) == vals24
t_solve, t_create = median3(lambda: s.solve(el24, lo24, hi24), 5), median3(create20, 5)
lines.append("\n[point]  16 elements in a span of 2^24 with a ready solver against eg_dlog_table_create over 2^20 values (create + destroy), medians of 5")
lines.append(f"point solve_ms {t_solve * 1e3:.3f} table_create_ms {t_create * 1e3:.1f} ratio {t_create / t_solve:.0f}")

lines.append("\n[chosen]  (csrc/dlog_host.hpp)")
lines.append(f"default baby_bits {bits}: {s.table_bytes >> 20} MiB of table, built in {build_ms[bits]:.1f} ms; every bit more halves the giant steps of a call and doubles "
             f"the table and its build ({build_ms[28]:.0f} ms and {4 << 10} MiB at 28), and no span an election produces needs it: "
             + (f"16 elements in a span of 2^48 take {worst_16_48 * 1e3:.0f} ms" if worst_16_48 else "see [solve]"))
lines.append(f"LAUNCH_LANES 2^{LAUNCH_LANES}: lanes of 64 giant steps per launch (two waves per SIMD), so that no launch is long and the host can stop between launches"
             + (f": {(64 << LAUNCH_LANES) / best_rate * 1e3:.2f} ms a launch at the best rate above" if best_rate else ""))
if best_rate:
    lines.append(f"CALL_STEPS 2^{CALL_STEPS}: giant steps a whole call may take = {(1 << CALL_STEPS) / best_rate:.1f} s at the best rate above "
                 f"({best_rate:.3e} giant steps per second); max_span(n) = CALL_STEPS / n * 2^baby_bits = 2^{s.max_span(1).bit_length() - 1} for one element")
s.close()
text = "\n".join(lines) + "\n"
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(text)
print(text, end="")
ctx.close()
