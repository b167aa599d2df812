"""Field, point and scalar arithmetic at the corners of the limb-bound discipline, on the GPU.

The device compilation of fe25519.cuh / ge25519.cuh / sc25519.cuh is not the host one: fe_twice is an inline v_add_u32, the multiply-add
chains are pinned by EG_SEED_FENCE, EG_SCHED_FENCE orders the multiplications.  tests/devcheck/devcheck.hip (a test-only library, built
by tests/devcheck/Makefile with the product's compiler flags) runs every operation on raw limb records, one lane per case.  Every batch of
tests/limb_cases.py - the records that tests/test_limb_corners_cpu.py runs through the bound-check host build - must give

* the operation on Python integers, bit for bit (Batch.check), and
* the very words the host build gives, limb for limb and not only mod p: two compilations of one header.

Every case is inside the stated preconditions (the host build has asserted that on the same records before the device sees them).
"""
import ctypes as C
import math
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import limb_cases as lc
from test_hostcheck import hc  # noqa: F401  (the host build the device is compared with)
from test_limb_corners_cpu import run_host

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent / "devcheck"
CSRC = HERE.parent.parent / "elastic_elgamal_amd" / "csrc"


def _flags(makefile):
    text = makefile.read_text()
    arch = re.search(r"^ARCH \?= (\S+)$", text, re.M).group(1)
    return re.search(r"^FLAGS = (.+)$", text, re.M).group(1).replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def dc(hc):  # noqa: F811
    subprocess.check_call(["make", "-C", str(HERE)], stdout=subprocess.DEVNULL)      # up to date when it travelled with the snapshot
    if "torch" not in sys.modules:          # one HIP runtime per process: the one of the PyTorch wheel, as the package itself does
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    d = C.CDLL(str(HERE / "libdevcheck.so"))
    assert d.dc_limb_op_count() == hc.hc_limb_op_count() == len(lc.OPS)
    return d


def run_dev(dc, b, rows=None, block=256):
    inp = b.inp if rows is None else np.ascontiguousarray(b.inp[rows])
    out = np.full_like(inp, 0xA5A5A5A5)
    step = C.c_int(0)
    status = dc.dc_limb_ops(C.c_int(b.op), C.c_int(len(inp)), inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                            C.c_int(block), C.byref(step))
    assert status == 0, f"{b.name}: HIP status {status} at step {step.value}"
    return out


def test_flags_are_the_products():
    """built exactly as the product is: the same FLAGS line, none of the EG_NO_* switches, no bound-check macros"""
    flags = _flags(HERE / "Makefile")
    assert flags == _flags(CSRC / "Makefile") == ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
    src = (HERE / "devcheck.hip").read_text() + (HERE / "limb_ops.cuh").read_text() + (HERE / "Makefile").read_text()
    assert "EG_NO_" not in src and "EG_BOUNDCHECK" not in src and "-D" not in (HERE / "Makefile").read_text()


@pytest.mark.parametrize("name", lc.MATRIX)
def test_every_case_on_the_device(dc, hc, name):  # noqa: F811
    b = lc.batch(name)
    assert len(b) >= 4096 and len(b) % 64 != 0          # several blocks and a partial last wavefront
    out = run_dev(dc, b)
    b.check(out)
    host = run_host(hc, b)
    diff = np.nonzero((out != host).any(axis=1))[0]
    assert diff.size == 0, (name, "device and host build differ in cases", diff[:8].tolist(), [b.names[i] for i in diff[:8]])


@pytest.mark.parametrize("name", ["mul", "sq", "sqn", "carry", "canon", "add_to_p3", "dbl_to_p3", "ge_add", "ge_madd", "ge_dbl"])
@pytest.mark.parametrize("block", [64, 256])
def test_lane_placement(dc, hc, name, block):  # noqa: F811
    """The corner case (all limbs at the top of the widest class - for fe_mul the largest class product - with slack) at lanes 0, 63, 64 and the last lane of a partial wavefront
    among random cases; a wavefront whose 64 lanes all hold it; a wavefront whose 64 lanes all differ."""
    b = lc.batch(name)
    rng = np.random.default_rng(lc.OPS[name] * 1000 + block)
    corner = max((i for i, fam in enumerate(b.names) if fam == "slack"), key=lambda i: (math.prod(b.classes[i]) if name == "mul" else sum(b.classes[i]), i))
    others = [i for i, fam in enumerate(b.names) if fam != "slack"]
    n = 3 * 64 + 17
    rows = rng.choice(others, n, replace=False)
    for lane in (0, 63, 64, n - 1):
        rows[lane] = corner
    launches = [rows.tolist(), [corner] * 64, rng.choice(len(b), 64, replace=False).tolist()]
    assert len(set(launches[2])) == 64
    for rows in launches:
        out = run_dev(dc, b, rows, block)
        b.check(out, rows)
        assert np.array_equal(out, run_host(hc, b, rows)), (name, block, len(rows))
