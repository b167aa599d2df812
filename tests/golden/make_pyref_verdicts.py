#!/usr/bin/env python3
"""Write tests/golden/pyref_verdicts.json: the verdicts of tests/pyref (the pure-Python verifier) on the corpus of
tests/pyref_cases.py -- per family pyref's status word of every case, a hash prefix of every case as lookup key, one SHA-256 over all the
cases' SHA-256 digests, and per election the SHA-256 of pyref's tally of the accepted cases (pyref_cases.fixture_entry).  The corpus is built by the oracle's provers, so this runs wherever the CPU suite runs (no GPU, no reference tree):

    python tests/golden/make_pyref_verdicts.py            # rewrite the fixture
    python tests/golden/make_pyref_verdicts.py --counts   # also print cases and seconds per family

tests/test_pyref_cpu.py regenerates every family at test time and compares it with the committed file.
"""
import json
import sys
import time
from pathlib import Path

TESTS = Path(__file__).resolve().parent.parent
for p in (str(TESTS), str(TESTS.parent)):
    if p not in sys.path:
        sys.path.insert(0, p)

import pyref_cases as PC  # noqa: E402


def build(report=None) -> dict:
    families = {}
    for corpus, name, key_name in PC.all_ids():
        t0, cpu0 = time.time(), PC.judge.cpu_seconds
        jf = PC.judged(corpus, name, key_name)
        t1 = time.time()
        families[jf.id] = PC.fixture_entry(jf)
        if report:
            report(jf, t1 - t0, time.time() - t1, PC.judge.cpu_seconds - cpu0)
    return {"_source": "tests/golden/make_pyref_verdicts.py: tests/pyref on the corpus of tests/pyref_cases.py",
            "families": families}


def dump(fixture: dict) -> str:
    """One family a line: the file stays diffable and small."""
    lines = ['{"_source": %s,' % json.dumps(fixture["_source"]), ' "families": {']
    fams = list(fixture["families"].items())
    for i, (k, v) in enumerate(fams):
        lines.append("  %s: %s%s" % (json.dumps(k), json.dumps(v, separators=(",", ":")), "," if i + 1 < len(fams) else ""))
    lines += [" }", "}"]
    return "\n".join(lines) + "\n"


def main() -> None:
    counts = "--counts" in sys.argv

    def report(jf, t_build, t_wall, t_pyref):
        print(f"{jf.id:34s} cases {len(jf.cases):5d}  build {t_build:5.1f} s  pyref {t_pyref:6.1f} s in {t_wall:5.1f} s on the pool", file=sys.stderr)

    fixture = build(report if counts else None)
    PC.FIXTURE.write_text(dump(fixture))
    n = sum(f["n"] for f in fixture["families"].values())
    print(f"wrote {PC.FIXTURE}: {len(fixture['families'])} families, {n} cases", file=sys.stderr)


if __name__ == "__main__":
    main()
