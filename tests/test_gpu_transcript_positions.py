"""The transcript layer (elastic_elgamal_amd/csrc/merlin.cuh) on the device at every position of the STROBE block: the script corpus of
tests/transcript_scripts.py (tests/test_transcript_positions_cpu.py says what it holds and proves with the position model that it
reaches every position) through tests/merlindev - merlin.cuh, unchanged, compiled with the product's flags behind the script
interpreter that the host build shares - over both LDS strides the product keeps a transcript state in: LdsState itself (stride NT)
and a policy of the small-batch kernel's stride (LdsStateT<SM_LANES>).  One script per launch, one case per lane, 65 cases with distinct messages (lanes 0, 63 and 64).

Every output word is compared with the oracle's independent transcript (oracle/transcript.c) and, word for word, with the bound-check
host build; the expected value never comes from merlin.cuh."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import transcript_scripts as ts
from test_hostcheck import hc  # noqa: F401  (the one host build, shared)
from test_transcript_positions_cpu import check_against_oracle, oracle_words, run_host

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent / "merlindev"
CSRC = HERE.parent.parent / "elastic_elgamal_amd" / "csrc"
POLICIES = {0: "LdsState, stride NT", 1: "stride SM_LANES of the small-batch kernel"}


def _flags(makefile):
    text = makefile.read_text()
    arch = re.search(r"^ARCH \?= (\S+)$", text, re.M).group(1)
    return re.search(r"^FLAGS = (.+)$", text, re.M).group(1).replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def md():
    subprocess.check_call(["make", "-C", str(HERE)], stdout=subprocess.DEVNULL)      # up to date when it travelled with the snapshot
    if "torch" not in sys.modules:          # one HIP runtime per process: the one of the PyTorch wheel, as the package itself does
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    d = C.CDLL(str(HERE / "libmerlindev.so"))
    d.md_run_script.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    return d


def run_dev(md, policy, name, script, msgs: bytes, n: int):
    blob = ts.encode(script)
    ow = ts.out_words(script)
    out = np.full((n, ow), 0xA5A5A5A5, dtype=np.uint32)
    step = C.c_int(0)
    status = md.md_run_script(policy, blob, len(blob), n, msgs, ts.msg_bytes(script), out.ctypes.data, ow, C.byref(step))
    assert status == 0, f"{name} ({POLICIES[policy]}): HIP status {status} at step {step.value}"
    return out


def test_flags_and_strides_are_the_products(md):
    """built exactly as the product is, and over the product's strides"""
    flags = _flags(HERE / "Makefile")
    assert flags == _flags(CSRC / "Makefile") == ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
    src = (HERE / "merlindev.hip").read_text() + (HERE / "transcript_script.cuh").read_text() + (HERE / "Makefile").read_text()
    assert "EG_NO_" not in src and "EG_BOUNDCHECK" not in src and "-D" not in (HERE / "Makefile").read_text()
    nt = int(re.search(r"^constexpr int NT = (\d+);", (CSRC / "device_io.cuh").read_text(), re.M).group(1))
    sm = int(re.search(r"^constexpr int SM_LANES = (\d+);", (CSRC / "latency_kernels.cuh").read_text(), re.M).group(1))
    assert (md.md_stride(0), md.md_stride(1)) == (nt, sm)
    assert md.md_lanes_per_block(0) > 64 and md.md_lanes_per_block(1) < ts.CASES          # lane 64, and a second block


def test_the_corpus_on_the_device(md, hc, oracle):  # noqa: F811
    for k, (name, script) in enumerate(ts.corpus() + ts.REGRESSIONS):
        msgs = ts.messages(script, ts.CASES, k)
        want = oracle_words(oracle, script, msgs, ts.CASES)
        host = run_host(hc, script, msgs, ts.CASES)
        for policy in POLICIES:
            got = run_dev(md, policy, name, script, msgs, ts.CASES)
            check_against_oracle(f"{name} ({POLICIES[policy]})", script, got, want)
            diff = np.argwhere(got != host)
            assert diff.size == 0, (name, POLICIES[policy], "device and host build differ at (case, word)", diff[:6].tolist())


@pytest.mark.parametrize("policy", list(POLICIES))
def test_one_launch_of_257_cases(md, hc, oracle, policy):  # noqa: F811
    """several blocks and a last block of one lane"""
    by_name = dict(ts.corpus())
    for name in ("label163", "tail333_proto0", "squeeze165_1"):
        script = by_name[name]
        msgs = ts.messages(script, 257, 99)
        got = run_dev(md, policy, name, script, msgs, 257)
        check_against_oracle(name, script, got, oracle_words(oracle, script, msgs, 257))
        assert (got == run_host(hc, script, msgs, 257)).all(), name


def test_a_script_outside_its_buffers_is_not_launched(md):
    script = [("init", b"x"), ("append_words", b"m", 0, 33), ("challenge64", b"c")]
    blob = ts.encode(script)
    out = np.zeros(16, dtype=np.uint32)
    step = C.c_int(0)
    INVALID = 1                                          # hipErrorInvalidValue
    assert md.md_run_script(0, blob, len(blob), 1, bytes(36), 32, out.ctypes.data, 16, C.byref(step)) == INVALID and step.value == 0
    assert md.md_run_script(0, blob, len(blob), 1, bytes(36), 36, out.ctypes.data, 15, C.byref(step)) == INVALID and step.value == 0
    assert md.md_run_script(2, blob, len(blob), 1, bytes(36), 36, out.ctypes.data, 16, C.byref(step)) == INVALID and step.value == 0
    assert md.md_run_script(1, blob, len(blob), 1, bytes(36), 36, out.ctypes.data, 16, C.byref(step)) == 0 and step.value == 7
