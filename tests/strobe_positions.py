"""Where every operation of a transcript program starts inside the 166-byte STROBE block (merlin.cuh: EG_STROBE_R).

A model of POSITIONS only - no Keccak, no bytes: `pos` and `pos_begin` as strobe_begin_op, strobe_absorb_byte, strobe_absorb_word
(with its byte-wise fallback when the word straddles the block end), merlin_frame and merlin_challenge64 move them.  Every operation
leaves an event (kind, start position), so that a test can ask which of the 166 positions a set of cases reaches.  The model is the
completeness condition of the transcript tests (tests/test_transcript_positions_cpu.py pins it to the oracle and to the host build of
merlin.cuh, and asserts that the cases of the sweeps reach every position).

Builders: the Transcript::new(label) prefix, the per-item programs of the sum-of-squares and commitment-equivalence proofs as
host_plan.hpp lays them out (build_sumsq_plan, build_commit_equiv_plan), and the scripts of tests/transcript_scripts.py."""
from __future__ import annotations

R = 166
META_AD, AD, PRF = 16 | 2, 2, 1 | 2 | 4
FLAG_NAMES = {META_AD: "meta_ad", AD: "ad", PRF: "prf"}


class Trace:
    def __init__(self):
        self.pos = 0
        self.pos_begin = 0
        self.events = []            # (kind, start position): begin_meta_ad / begin_ad / begin_prf / absorb_word / absorb_word_bytes /
        #                             squeeze_word / squeeze_word_bytes / frame_label_cross / frame_len_cross / forced_f / skipped_f
        self.between_ops = []       # (pos, pos_begin) after each whole operation of a program
        self.pos_words = []         # pos | pos_begin << 8 at each ("pos",) of a script

    # ---- STROBE ----
    def _run_f(self):
        self.pos = 0
        self.pos_begin = 0

    def byte(self):                 # strobe_absorb_byte / strobe_squeeze_byte
        self.pos += 1
        if self.pos == R:
            self._run_f()

    def bytes(self, n):
        for _ in range(n):
            self.byte()

    def begin_op(self, flags):
        self.events.append(("begin_" + FLAG_NAMES[flags], self.pos))
        self.pos_begin = self.pos + 1
        self.byte()
        self.byte()
        if flags & (4 | 32):
            if self.pos != 0:
                self.events.append(("forced_f", self.pos))
                self._run_f()
            else:
                self.events.append(("skipped_f", 0))

    def _word(self, kind):
        if self.pos + 4 <= R:
            self.events.append((kind, self.pos))
            self.pos += 4
            if self.pos == R:
                self._run_f()
        else:
            self.events.append((kind, self.pos))
            self.events.append((kind + "_bytes", self.pos))
            self.bytes(4)

    def absorb_word(self):
        self._word("absorb_word")

    def squeeze_word(self):
        self._word("squeeze_word")

    def absorb_words(self, n_bytes):            # strobe_absorb_words: whole words, then the tail byte by byte
        for _ in range(n_bytes >> 2):
            self.absorb_word()
        self.bytes(n_bytes & 3)

    # ---- Merlin ----
    def frame(self, label_len):
        self.begin_op(META_AD)
        if label_len >= 2 and self.pos + label_len > R:
            self.events.append(("frame_label_cross", self.pos))
        self.bytes(label_len)
        if self.pos + 4 > R:
            self.events.append(("frame_len_cross", self.pos))
        self.bytes(4)

    def append_bytes(self, label_len, n):
        self.frame(label_len)
        self.begin_op(AD)
        self.bytes(n)

    def append_words(self, label_len, n):
        self.frame(label_len)
        self.begin_op(AD)
        self.absorb_words(n)

    def append_u64(self, label_len):
        self.append_bytes(label_len, 8)

    def challenge64(self, label_len):
        self.frame(label_len)
        self.begin_op(PRF)
        for _ in range(16):
            self.squeeze_word()

    def squeeze(self, label_len, k, m):
        self.frame(label_len)
        self.begin_op(PRF)
        self.bytes(k)
        for _ in range(m):
            self.squeeze_word()

    def init(self, label_len):                  # merlin_init: "Merlin v1.0" as meta-AD, then append_message("dom-sep", label)
        self.pos = 0
        self.pos_begin = 0
        self.begin_op(META_AD)
        self.bytes(11)
        self.append_bytes(7, label_len)

    def op_done(self):
        self.between_ops.append((self.pos, self.pos_begin))

    # ---- queries ----
    def starts(self, kind):
        return {p for k, p in self.events if k == kind}


def merge(traces):
    t = Trace()
    for x in traces:
        t.events += x.events
        t.between_ops += x.between_ops
    return t


def prefix(label_len: int) -> Trace:
    t = Trace()
    t.init(label_len)
    t.op_done()
    return t


def _wire(t: Trace, label: str, items: int = 1):          # OP_APPEND_WIRE / OP_APPEND_CMP: a frame, then 32-byte word absorbs
    t.frame(len(label))
    t.begin_op(AD)
    for _ in range(items):
        t.absorb_words(32)
    t.op_done()


def _blob(t: Trace, label: str, n: int):                  # OP_APPEND_BLOB: merlin_append_bytes
    t.append_bytes(len(label), n)
    t.op_done()


def sumsq_program(label_len: int, n: int) -> Trace:
    """build_sumsq_plan: the prefix program (saved and loaded through merlin_export / merlin_import, which keep the position) and the
    item's program after it."""
    t = prefix(label_len)
    _blob(t, "dom-sep", len("sum_of_squares"))
    _blob(t, "K", 32)
    for _ in range(n):
        for label in ("R_x", "X", "[e_r]G", "[e_x]G + [e_r]K"):
            _wire(t, label)
    for label in ("R_z", "Z", "[e_x]R_x + [e_z]G", "[e_x]X + [e_z]K"):
        _wire(t, label)
    t.challenge64(len("c"))
    t.op_done()
    return t


def commit_equiv_program(label_len: int) -> Trace:
    """build_commit_equiv_plan, prefix program and item program."""
    t = prefix(label_len)
    _blob(t, "dom-sep", len("commitment_equivalence"))
    _blob(t, "K", 32)
    for label in ("R", "B", "C", "[e_r]G", "[e_v]G + [e_r]K", "[e_v]G + [e_c]H"):
        _wire(t, label)
    t.challenge64(len("c"))
    t.op_done()
    return t


def run_script(script) -> Trace:
    """A script of tests/transcript_scripts.py: tuples (op name, ...) with labels as bytes."""
    t = Trace()
    for op in script:
        name = op[0]
        if name == "init":
            t.init(len(op[1]))
        elif name == "append_bytes":
            t.append_bytes(len(op[1]), op[3])
        elif name == "append_words":
            t.append_words(len(op[1]), op[3])
        elif name == "append_u64":
            t.append_u64(len(op[1]))
        elif name == "challenge64":
            t.challenge64(len(op[1]))
        elif name == "squeeze":
            t.squeeze(len(op[1]), op[2], op[3])
        elif name == "pos":
            t.pos_words.append(t.pos | (t.pos_begin << 8))
        elif name in ("export_import", "clone"):
            pass
        else:
            raise ValueError(name)
        if name not in ("pos",):
            t.op_done()
    return t


def legacy_merlin_sweep() -> Trace:
    """What tests/test_hostcheck.py::test_merlin runs (hc_merlin): one protocol label, the message length varies."""
    out = []
    for n in (0, 1, 31, 32, 64, 100, 165, 166, 167, 400):
        t = Trace()
        t.init(len("encrypted_choice_ranges"))
        t.append_words(len("enc"), n)
        t.append_u64(len("i"))
        t.challenge64(len("c"))
        out.append(t)
    t = Trace()
    t.init(len("test protocol"))
    t.append_words(len("some label"), 9)
    t.challenge64(len("challenge"))
    out.append(t)
    return merge(out)
