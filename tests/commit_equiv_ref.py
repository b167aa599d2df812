"""Test-side restatement of CommitmentEquivalenceProof::new / ::verify (src/proofs/commitment.rs:134-238) on the primitives of
oracle/oracle.py, with the engine's precedence of malformed items in front, so that `verify` returns the full status word of
eg_verify_proof_batch for ANY 224 bytes.

Item layout (include/eg_hip.h): R || B || C || challenge || randomness_response || value_response || commitment_response.
Draw order of the prover after `rng_skip` 64-byte draws (tests/snapshots.rs:163-177): r (CiphertextWithValue::new), r_c
(SecretKey::generate), e_r, e_v, e_c; every draw is fill_bytes(64) and a wide reduction."""
from __future__ import annotations

import json
from pathlib import Path

from oracle import oracle as o

ITEM = 224
N_POINTS, N_ITEMS = 3, 7
OK, BAD_SCALAR, BAD_POINT, CHALLENGE = 0, 1, 2, 4       # EG_ST_OK / _BAD_SCALAR / _BAD_POINT / _SUM_CHALLENGE
ZERO = bytes(32)
ONE = (1).to_bytes(32, "little")


def fixture() -> dict:
    return json.loads((Path(__file__).resolve().parent / "golden" / "commitment_equiv_ristretto.json").read_text())


def sc(x: int) -> bytes:
    return (x % o.L).to_bytes(32, "little")


def _fixed(scalars, points) -> bytes:
    """sum [k_i]P_i; G is given as None."""
    ks = b"".join(k for k, p in zip(scalars, points) if p is not None)
    ps = b"".join(p for p in points if p is not None)
    g = [k for k, p in zip(scalars, points) if p is None]
    acc = o.point_mul_generator(g[0]) if g else ZERO
    if ks:
        acc = o.point_add(acc, o.point_multi_mul(ks, ps))
    return acc


def prove(pk: bytes, h: bytes, label: bytes, value: int, rng, pins: dict | None = None):
    """(item, r_c).  `pins` replaces drawn scalars by name ("r", "r_c", "e_r", "e_v", "e_c"); the stream advances all the same."""
    pins = pins or {}
    draw = {}
    for name in ("r", "r_c", "e_r", "e_v", "e_c"):
        d = o.sc_from_wide(o.rng_fill64(rng))
        draw[name] = sc(pins[name]) if name in pins else d
    v = sc(value)
    R = o.point_mul_generator(draw["r"])
    B = _fixed([v, draw["r"]], [None, pk])
    C = _fixed([v, draw["r_c"]], [None, h])
    t = o.Merlin(label)
    t.append(b"dom-sep", b"commitment_equivalence")
    t.append(b"K", pk)
    t.append(b"R", R)
    t.append(b"B", B)
    t.append(b"C", C)
    t.append(b"[e_r]G", o.point_mul_generator(draw["e_r"]))
    t.append(b"[e_v]G + [e_r]K", _fixed([draw["e_v"], draw["e_r"]], [None, pk]))
    t.append(b"[e_v]G + [e_c]H", _fixed([draw["e_v"], draw["e_c"]], [None, h]))
    c = o.sc_from_wide(t.challenge(b"c", 64))
    s_r = o.sc_add(o.sc_mul(c, draw["r"]), draw["e_r"])
    s_v = o.sc_add(o.sc_mul(c, v), draw["e_v"])
    s_c = o.sc_add(o.sc_mul(c, draw["r_c"]), draw["e_c"])
    return R + B + C + c + s_r + s_v + s_c, draw["r_c"]


def verify(pk: bytes, h: bytes, label: bytes, item: bytes) -> int:
    """The status word eg_verify_proof_batch gives this item."""
    assert len(item) == ITEM
    it = [item[32 * i : 32 * i + 32] for i in range(N_ITEMS)]
    # the engine's precedence: the smallest (item * 4 + kind) among malformed items, i.e. the first malformed item in wire order
    for i in range(N_ITEMS):
        if i < N_POINTS:
            if o.point_roundtrip(it[i]) is None:
                return o.status(BAD_POINT, i)
        elif not o.sc_is_canonical(it[i]):
            return o.status(BAD_SCALAR, i)
    R, B, C, c, s_r, s_v, s_c = it
    neg_c = o.sc_neg(c)
    t = o.Merlin(label)
    t.append(b"dom-sep", b"commitment_equivalence")
    t.append(b"K", pk)
    t.append(b"R", R)
    t.append(b"B", B)
    t.append(b"C", C)
    t.append(b"[e_r]G", o.point_double_mul_generator(neg_c, R, s_r))
    t.append(b"[e_v]G + [e_r]K", o.point_add(o.point_mul_generator(s_v), o.point_multi_mul(s_r + neg_c, pk + B)))
    t.append(b"[e_v]G + [e_c]H", o.point_add(o.point_mul_generator(s_v), o.point_multi_mul(s_c + neg_c, h + C)))
    return OK if o.sc_from_wide(t.challenge(b"c", 64)) == c else CHALLENGE


def verify_many(pk: bytes, h: bytes, label: bytes, items: bytes) -> list:
    return [verify(pk, h, label, items[k : k + ITEM]) for k in range(0, len(items), ITEM)]


def _verify_slab(args):
    return verify_many(*args)


def verify_parallel(pk: bytes, h: bytes, label: bytes, items: bytes, workers: int = 16) -> list:
    """verify_many over EVERY item, on up to 16 processes."""
    import concurrent.futures as cf

    n = len(items) // ITEM
    per = max(1, (n + workers * 8 - 1) // (workers * 8))
    slabs = [(pk, h, label, items[k * ITEM : (k + per) * ITEM]) for k in range(0, n, per)]
    with cf.ProcessPoolExecutor(max_workers=min(workers, 16)) as ex:
        out = []
        for part in ex.map(_verify_slab, slabs):
            out += part
    assert len(out) == n
    return out
