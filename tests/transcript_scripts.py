"""The transcript script corpus of tests/test_transcript_positions_cpu.py and tests/test_gpu_transcript_positions.py, its binary form
for tests/merlindev/transcript_script.cuh, and what the oracle's independent transcript (oracle/transcript.c) gives for a script.

A script is a list of tuples; labels are bytes without NUL (the oracle takes C strings); `off` is a byte offset (a multiple of 4) into
the case's message area, so that every case of a launch runs the same program over its own message bytes:
    ("init", label)                    Transcript::new(label)
    ("append_bytes", label, off, n)    append_message through merlin_append_bytes
    ("append_words", label, off, n)    append_message through merlin_append_words (4 bytes at a time, a tail byte by byte)
    ("append_u64", label, off)         append_u64 of the 8 message bytes at off
    ("challenge64", label)             challenge_bytes(label, 64) through merlin_challenge64           -> 16 words
    ("squeeze", label, k, m)           challenge_bytes(label, k + 4 m): k bytes one by one, then m words -> ceil(k / 4) + m words
    ("export_import",)                 merlin_export, then merlin_import into the other (scrubbed) transcript, which goes on
    ("clone",)                         merlin_clone into the other (scrubbed) transcript, which goes on
    ("pos",)                           pos | pos_begin << 8                                              -> 1 word
"""
from __future__ import annotations

import random
import struct

OPS = {"init": 1, "append_bytes": 2, "append_words": 3, "append_u64": 4, "challenge64": 5, "squeeze": 6, "export_import": 7,
       "clone": 8, "pos": 9}
CASES = 65                       # per launch: lanes 0, 63 and 64
WORD_TAIL_LENGTHS = (0, 1, 3, 4, 5, 31, 33, 165, 166, 167, 332, 333)
# label lengths of the two label-carrying proof kinds on the GPU (tests/test_gpu_label_sweep.py); the model test decides whether
# the set is enough
PROOF_LABEL_LENGTHS = tuple(range(256))


def label_bytes(n: int, seed: int) -> bytes:
    """n bytes from 1..255, at least one of them >= 0x80."""
    rnd = random.Random(1000 * seed + n)
    b = bytearray(rnd.randrange(1, 256) for _ in range(n))
    if n and max(b) < 0x80:
        b[rnd.randrange(n)] = rnd.randrange(0x80, 256)
    return bytes(b)


def encode(script) -> bytes:
    """n_ops, then (op, label offset << 12 | label length, b, c) per operation as little-endian words, then the label bytes."""
    head = 4 + 16 * len(script)
    pool = bytearray()
    words = [len(script)]
    for op in script:
        name = op[0]
        label = op[1] if len(op) > 1 and isinstance(op[1], bytes) else b""
        assert len(label) <= 255 and 0 not in label
        ref = ((head + len(pool)) << 12) | len(label)
        pool += label
        b, c = (op[2], op[3]) if name in ("append_bytes", "append_words", "squeeze") else (op[2], 0) if name == "append_u64" else (0, 0)
        words += [OPS[name], ref, b, c]
    blob = struct.pack(f"<{len(words)}I", *words) + bytes(pool)
    return blob + bytes(-len(blob) % 4)


def out_words(script) -> int:
    n = 0
    for op in script:
        n += {"challenge64": 16, "pos": 1}.get(op[0], 0)
        if op[0] == "squeeze":
            n += (op[2] + 3) // 4 + op[3]
    return n


def msg_bytes(script) -> int:
    """Size of a case's message area: what the script reads, rounded up to whole words, at least one word."""
    need = 4
    for op in script:
        if op[0] in ("append_bytes", "append_words"):
            need = max(need, op[2] + (op[3] + 3) // 4 * 4)
        elif op[0] == "append_u64":
            need = max(need, op[2] + 8)
    return need


def messages(script, n_cases: int, seed: int) -> bytes:
    """Distinct message areas for the cases of one launch."""
    rnd = random.Random(seed)
    per = msg_bytes(script)
    out = bytearray(rnd.getrandbits(8 * per * n_cases).to_bytes(per * n_cases, "little"))
    for i in range(n_cases):                       # distinct even where the area is one word
        out[per * i : per * i + 2] = struct.pack("<H", i)
    return bytes(out)


def _pack(b: bytes) -> list:
    b = b + bytes(-len(b) % 4)
    return list(struct.unpack(f"<{len(b) // 4}I", b))


def expected(oracle, script, msg: bytes):
    """(output words, final pos) of the oracle's UNINTERRUPTED transcript: export/import and clone change nothing.  A ("pos",)
    word is the oracle's pos alone: compare it with the low byte (tests/strobe_positions.py gives the whole word)."""
    t, out = None, []
    for op in script:
        name = op[0]
        if name == "init":
            t = oracle.Merlin(op[1])
        elif name in ("append_bytes", "append_words"):
            t.append(op[1], msg[op[2] : op[2] + op[3]])
        elif name == "append_u64":
            t.append_u64(op[1], int.from_bytes(msg[op[2] : op[2] + 8], "little"))
        elif name == "challenge64":
            out += _pack(t.challenge(op[1], 64))
        elif name == "squeeze":
            k, m = op[2], op[3]
            b = t.challenge(op[1], k + 4 * m)
            out += _pack(b[:k]) + _pack(b[k:])
        elif name == "pos":
            out.append(t.pos)
    return out, t.pos


def pos_word_indices(script):
    """Indices of the ("pos",) words in the output."""
    idx, n = [], 0
    for op in script:
        if op[0] == "pos":
            idx.append(n)
        n += {"challenge64": 16, "pos": 1}.get(op[0], 0)
        if op[0] == "squeeze":
            n += (op[2] + 3) // 4 + op[3]
    return idx


def _interrupt(script, first: int):
    """export/import and clone, alternately, after every operation of the script."""
    out = []
    k = first
    for op in script:
        out.append(op)
        if op[0] != "pos":
            out.append(("export_import",) if k % 2 == 0 else ("clone",))
            k += 1
    return out


def corpus():
    """[(name, script)].  Protocol labels of every length 0..255 shift every later operation by one position each; the word appends
    are the 32- and 64-byte ones of the proof programs; the tails, append_u64 and the squeezes are as the module docstring of
    tests/test_transcript_positions_cpu.py lists them."""
    out = []
    for n in range(256):
        proto = label_bytes(n, 1)
        s = [("init", proto), ("append_words", label_bytes(1 + n % 3, 2), 0, 32)]
        if n % 2:
            s.append(("append_words", label_bytes(6, 3), 32, 32))
        s += [("append_words", label_bytes(15 + n % 4, 4), 64, 64), ("append_u64", label_bytes(1, 5), 128),
              ("append_bytes", label_bytes(2, 18), 0, 0), ("pos",), ("challenge64", label_bytes(1, 6)), ("pos",), ("challenge64", label_bytes(2, 7))]
        out.append((f"label{n}", _interrupt(s, n)))
    for pi, pn in enumerate((0, 13, 150)):
        for n in WORD_TAIL_LENGTHS:
            s = [("init", label_bytes(pn, 8)), ("append_words", label_bytes(3, 9), 0, n), ("append_bytes", label_bytes(2, 10), 0, n),
                 ("append_words", label_bytes(4, 11), 4, n), ("append_u64", label_bytes(1, 12), 8), ("pos",),
                 ("challenge64", label_bytes(1, 13))]
            out.append((f"tail{n}_proto{pn}", s if pi else _interrupt(s, n)))
    for k in range(170):
        m = 1 + k % 3
        s = [("init", label_bytes(k, 14)), ("append_bytes", label_bytes(1, 19), 0, 0), ("export_import",), ("clone",), ("pos",),
             ("append_bytes", label_bytes(1, 15), 0, 5 + k % 7),
             ("squeeze", label_bytes(1 + k % 2, 16), k, m), ("pos",), ("challenge64", label_bytes(1, 17))]
        out.append((f"squeeze{k}_{m}", s))
    return out


# a named regression case per script that once failed goes here: (name, script)
REGRESSIONS = []
