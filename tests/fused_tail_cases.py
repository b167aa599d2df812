"""The batches of tests/test_gpu_encode_hash_fused.py (test infrastructure) and the routine that runs one of them on the GPU."""
from __future__ import annotations

import functools
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import edge_ballots as E  # noqa: E402

SIZES = (1, 2, 3, 63, 64, 65, 129, 257)


def tamper_response(ballot: bytes) -> bytes:
    """One response bit flipped, the one bench.py --tampered-percent flips."""
    b = bytearray(ballot)
    b[len(b) - 32] ^= 1
    return bytes(b)


def _split(fam, raw):
    return [raw[i : i + fam.size] for i in range(0, len(raw), fam.size)]


def guard_edges(fam):
    """The edge ballots with commitments that are the identity: their encodings go through the encoder's vanishing-denominator guard."""
    return [e.ballot for e in fam.edges if "commitment" in e.needs]


@functools.lru_cache(None)
def cases() -> dict:
    """name -> (family name, ballots, environment of the params object, entry)."""
    out = {}
    s5 = E.family("single5")
    rand = _split(s5, s5.random_ballots(9001, 257))
    for n in SIZES:
        out[f"size{n}"] = ("single5", rand[:n], {}, "batch")
    for name in ("single2", "single7", "single8", "multi3of16", "qv5x20"):
        fam = _family(name)
        b = _split(fam, fam.random_ballots(9002, 65))
        b[5] = tamper_response(b[5])
        out[f"options_{name}"] = (name, b, {}, "batch")
    # a batch of 65: lane 0 owns ballots 0 and 33
    for tag, bad in (("first", (0,)), ("partner", (33,)), ("both", (0, 33))):
        b = list(rand[:65])
        for i in bad:
            b[i] = tamper_response(b[i])
        out[f"tampered_{tag}"] = ("single5", b, {}, "batch")
    # guard ballots paired with ordinary ones (both ways round) and with each other
    g = guard_edges(s5)
    k = len(g)
    out["edge_first"] = ("single5", g + rand[:k], {}, "batch")
    out["edge_second"] = ("single5", rand[:k] + g, {}, "batch")
    out["edge_both"] = ("single5", g + g[1:] + g[:1], {}, "batch")
    out["edge_odd"] = ("single5", g + rand[: k - 1], {}, "batch")          # the last guard ballot alone in its lane
    # chunks: the engine cuts a call into chunks that are multiples of its block of 256 ballots, so 130 ballots stay one chunk whatever
    # EG_CHUNK says; 386 = 256 + 130 gives two chunks, one after the other on one work set (batch entry) and one on each work set
    # (the JSON entry always forks)
    b130 = rand[:130]
    out["chunk_130"] = ("single5", b130, {"EG_CHUNK": "65"}, "batch")
    b386 = rand[:257] + [tamper_response(x) if i % 50 == 0 else x for i, x in enumerate(rand[:129])]
    out["chunk_386"] = ("single5", b386, {"EG_CHUNK": "256"}, "batch")
    out["chunk_386_two_sets"] = ("single5", b386, {"EG_CHUNK": "256"}, "json")
    return out


@functools.lru_cache(None)
def _family(name):
    """single5 with its edge corpus; the other elections plain (ordinary ballots only)."""
    if name == "single5":
        return E.family(name)
    from oracle import oracle as o

    pk = E.key("golden")
    if name == "qv5x20":
        fam = E.Family(name, "qv", "golden", pk, n_options=5, credits=20, oracle_params=o.QvParams(pk, 5, 20))
    elif name == "multi3of16":
        fam = E.Family(name, "multi", "golden", pk, n_options=16, oracle_params=o.ChoiceParams(pk, 16, False))
    else:
        n = int(name[6:])
        fam = E.Family(name, "single", "golden", pk, n_options=n, oracle_params=o.ChoiceParams(pk, n, True))
    fam.edges.append(E.Edge("plain", fam.random_ballots(77, 1)))      # Family.size reads the first edge
    return fam


def family_of(case_name):
    return _family(cases()[case_name][0])


def run_case(eg, ctx, name):
    """(status words, tally bytes as hex) of one case on the GPU."""
    fam_name, ballots, env, entry = cases()[name]
    fam = _family(fam_name)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                       # read when the params object is made
    try:
        p = fam.gpu_params(eg, ctx)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        if entry == "json":
            from elastic_elgamal_amd import serde

            objs = [serde.unpack_encrypted_choice(b, fam.n_options, True) for b in ballots]
            st, tally = p.verify_json(json.dumps(objs))
        else:
            st, tally = p.verify_batch(b"".join(ballots))
        return list(st), tally.hex()
    finally:
        p.close()
