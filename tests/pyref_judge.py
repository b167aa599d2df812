"""Runs tests/pyref over many inputs on a pool of processes (test infrastructure).  The workers are SPAWNED and this module imports
nothing but pyref and the standard library, so a worker never holds the oracle, the product library or a GPU."""
from __future__ import annotations

import atexit
import concurrent.futures as cf
import functools
import json
import multiprocessing
import os
import time

from pyref import objects, packed


@functools.lru_cache(None)
def verifier(spec: tuple):
    """spec = (kind, the constructor's arguments...): single / multi (key, options), qv (key, options, credits), zero / bool (key),
    range (key, bound), share (shared key, shares, threshold, index, participant key), sumsq (key, values, label), commit_equiv (key,
    blinding base, label)."""
    kind, args = spec[0], spec[1:]
    if kind in ("single", "multi"):
        return packed.ChoiceVerifier(args[0], args[1], kind == "single")
    return {"qv": packed.QvVerifier, "zero": packed.ZeroVerifier, "bool": packed.BoolVerifier, "range": packed.RangeVerifier,
            "share": packed.ShareVerifier, "sumsq": packed.SumOfSquaresVerifier,
            "commit_equiv": packed.CommitmentEquivalenceVerifier}[kind](*args)


def _words(spec, blobs):
    if spec[0] == "object":                              # ("object", kind, key, options, credits); the blobs are JSON texts
        _, kind, key, n, credits = spec
        if kind == "qv":
            return [objects.verify_qv(key, n, credits, json.loads(b)) for b in blobs]
        return [objects.verify_choice(key, n, kind == "single", json.loads(b)) for b in blobs]
    v = verifier(spec)
    return [v.verify(b) for b in blobs]


def _slab(args):
    t0 = time.process_time()
    return _words(*args), time.process_time() - t0


_pool = None


def pool() -> cf.ProcessPoolExecutor:
    global _pool
    if _pool is None:
        _pool = cf.ProcessPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1)), mp_context=multiprocessing.get_context("spawn"))
        atexit.register(_pool.shutdown)                  # the workers end with the interpreter, before its modules are torn down
    return _pool


def judge(spec: tuple, blobs: list) -> list:
    """pyref's status word of every blob, in order."""
    per = max(1, min(16, len(blobs) // 32 or 1))
    slabs = [(spec, blobs[i : i + per]) for i in range(0, len(blobs), per)]
    out = []
    for part, seconds in pool().map(_slab, slabs):
        out += part
        judge.cpu_seconds += seconds
    return out


judge.cpu_seconds = 0.0                                  # pyref time spent so far, summed over the pool's processes
