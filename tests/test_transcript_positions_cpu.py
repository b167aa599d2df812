"""The transcript layer (elastic_elgamal_amd/csrc/merlin.cuh) at every position of the 166-byte STROBE block, without a GPU.

* tests/strobe_positions.py models where each operation of a transcript program starts.  It is pinned to the code here: for every
  script of the corpus the position it predicts is the oracle's (oracle/transcript.c) and the one the host build of merlin.cuh returns.
* The model then is the completeness condition of the sweeps: the label lengths of tests/test_gpu_label_sweep.py for the two proof kinds
  that take a caller's label, and the script corpus (tests/transcript_scripts.py), each reach all 166 start positions of
  begin_op(META_AD), begin_op(AD) and begin_op(PRF), all 166 start positions of a 4-byte absorb (163, 164 and 165, where it falls back
  to bytes, among them), and frames whose label bytes and whose four length bytes cross a block.
* The whole corpus runs through the script interpreter (tests/merlindev/transcript_script.cuh) in the bound-check / UBSan host build
  over ArrState, 65 cases with distinct messages per script, and every output word is the oracle's.

Corpus: protocol labels of 0..255 bytes (bytes 1..255, one >= 0x80 at least) in front of one or two 32-byte and one 64-byte word
append, append_u64 and two challenges, with export -> import and clone after every operation; word appends of 0, 1, 3, 4, 5, 31, 33,
165, 166, 167, 332 and 333 bytes (the tail path of strobe_absorb_words) next to the byte form; challenge_bytes(k + 4 m) squeezed as k
single bytes (0..169) and m words (1..3), which takes strobe_squeeze_word through every alignment and across the block end."""
import ctypes as C

import numpy as np
import pytest

import strobe_positions as sp
import transcript_scripts as ts
from test_hostcheck import hc  # noqa: F401  (the one host build, shared)

ALL = set(range(sp.R))


def run_host(hc, script, msgs: bytes, n: int):
    blob = ts.encode(script)
    per, ow = ts.msg_bytes(script), ts.out_words(script)
    out = np.zeros((n, ow), dtype=np.uint32)
    hc.hc_transcript_script.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
    assert hc.hc_transcript_script(blob, len(blob), n, msgs, per, out.ctypes.data, ow) == 0
    return out


def oracle_words(oracle, script, msgs: bytes, n: int):
    """What the oracle's transcript gives for the n cases, as an array like the outputs'."""
    per = ts.msg_bytes(script)
    return np.array([ts.expected(oracle, script, msgs[per * i : per * (i + 1)])[0] for i in range(n)], dtype=np.uint32).reshape(n, -1)


def check_against_oracle(name, script, got, want):
    """Every output word of every case against the oracle's; a ("pos",) word holds pos_begin too, which only the model knows."""
    got = got.copy()
    model = sp.run_script(script)
    for k, j in enumerate(ts.pos_word_indices(script)):
        assert (got[:, j] == model.pos_words[k]).all(), (name, "pos word", k, hex(int(got[0, j])), hex(model.pos_words[k]))
        got[:, j] &= 0xFF
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, "(case, word) that differ from the oracle", bad[:6].tolist())


def op_starts(t):
    return t.starts("begin_meta_ad") | t.starts("begin_ad") | t.starts("begin_prf")


def test_the_model_reproduces_the_coverage_figures_of_the_old_sweeps():
    """The positions reached BEFORE this corpus, from the model: the message-length sweep of test_hostcheck.py::test_merlin, and the
    proof programs under the labels of 4 and 10 bytes that the suite used (distinct positions out of 166)."""
    old = sp.legacy_merlin_sweep()
    assert (len(op_starts(old)), len(old.starts("absorb_word"))) == (39, 85)
    assert not op_starts(old) & {164, 165} and old.starts("absorb_word_bytes") == {164}
    ce = sp.merge([sp.commit_equiv_program(4), sp.commit_equiv_program(10)])
    assert (len(op_starts(ce)), len(ce.starts("absorb_word"))) == (37, 81)
    assert len(sp.commit_equiv_program(4).starts("begin_prf")) == 1                 # one position for the challenge per label length
    assert len(op_starts(sp.merge([sp.sumsq_program(4, n) for n in (1, 2, 5, 16)]))) == 130
    # a PRF operation forces a permutation first, so the shipped programs squeeze words at 0, 4, ... 60 only
    assert ce.starts("squeeze_word") == set(range(0, 64, 4))


def complete(t: sp.Trace, what: str):
    for kind in ("begin_meta_ad", "begin_ad", "begin_prf", "absorb_word"):
        assert t.starts(kind) == ALL, (what, kind, sorted(ALL - t.starts(kind)))
    assert t.starts("absorb_word_bytes") == {163, 164, 165}, what
    assert t.starts("frame_label_cross") and t.starts("frame_len_cross") >= {163, 164, 165}, what
    assert ("skipped_f", 0) in t.events and t.starts("forced_f"), what            # both sides of the `pos != 0` guard


def test_the_sweeps_reach_every_position():
    lengths = ts.PROOF_LABEL_LENGTHS
    assert 0 in lengths and 255 in lengths
    complete(sp.merge([sp.sumsq_program(n, v) for n in lengths for v in (1, 2)]), "sum of squares")
    complete(sp.merge([sp.commit_equiv_program(n) for n in lengths]), "commitment equivalence")
    corpus = sp.merge([sp.run_script(s) for _, s in ts.corpus()])
    complete(corpus, "script corpus")
    # strobe_squeeze_word: every alignment, and the fallback at each of its three positions
    assert corpus.starts("squeeze_word") == ALL
    assert corpus.starts("squeeze_word_bytes") == {163, 164, 165}
    # export / import and clone see every position and every pos_begin an operation can leave behind: a header that starts at 164 or
    # 165 wraps the block, which resets pos_begin, so 164 (an empty message begun at 163) is the largest
    assert {p for p, _ in corpus.between_ops} == ALL
    assert {b for _, b in corpus.between_ops} == set(range(0, 165))


def test_the_model_is_the_code(hc, oracle):
    """Position by position: model == oracle == host build, for one case of every script of the corpus."""
    for name, script in ts.corpus() + ts.REGRESSIONS:
        model = sp.run_script(script)
        msgs = ts.messages(script, 1, 7)
        _, pos = ts.expected(oracle, script, msgs)
        assert model.pos == pos, name
        got = run_host(hc, script + [("pos",)], msgs, 1)
        assert int(got[0, -1]) == (model.pos | (model.pos_begin << 8)), name
        assert int(got[0, -1]) & 0xFF == pos, name


def test_the_host_build_runs_the_whole_corpus_like_the_oracle(hc, oracle):
    for k, (name, script) in enumerate(ts.corpus() + ts.REGRESSIONS):
        msgs = ts.messages(script, ts.CASES, k)
        got = run_host(hc, script, msgs, ts.CASES)
        check_against_oracle(name, script, got, oracle_words(oracle, script, msgs, ts.CASES))


def test_scripts_that_do_not_fit_their_buffers_are_refused(hc):
    script = [("init", b"x"), ("append_words", b"m", 0, 33), ("challenge64", b"c")]
    blob = ts.encode(script)
    out = np.zeros(16, dtype=np.uint32)
    hc.hc_transcript_script.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
    run = lambda blob, per, ow: hc.hc_transcript_script(blob, len(blob), 1, bytes(64), per, out.ctypes.data, ow)
    assert run(blob, 36, 16) == 0
    assert run(blob, 32, 16) == -1                    # the tail byte's word lies outside the message area
    assert run(blob, 36, 15) == -1                    # output of another size
    assert run(blob[:-4], 36, 16) == -1               # a label outside the blob
    assert run(ts.encode(script[1:]), 36, 16) == -1   # no transcript yet
