"""The fused square-and-subtract, the chain doubling, the comb product with the sign on the accumulator and the fixed comb's zero-digit
path, on the GPU.

* tests/dblchaindev (a test-only library, built by its Makefile with the product's compiler flags) runs the records of
  tests/dbl_chain_cases.py, one lane per case in a single launch: the operation on Python integers, and limb for limb the words of
  the bound-check host build of the same header (tests/hostcheck/dblchaincheck.cpp, which has run the same records first, so every
  case is inside the stated preconditions).  The same library runs ge_teeth_mul over a table in device memory, one lane per scalar.
* the product library: [k]P + [r]G (vartime_multi_mul_device with one term: the fixed comb adds [r]G to the variable-base product)
  and batches of ballots of every comb shape, byte for byte against the oracle.
"""
import ctypes as C
import random
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import dbl_chain_cases as dcc
from test_dbl_chain_cpu import prog, run, run_records  # noqa: F401  (the host build the device is compared with)

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent / "dblchaindev"
CSRC = HERE.parent.parent / "elastic_elgamal_amd" / "csrc"
L = dcc.L


def _flags(makefile):
    text = makefile.read_text()
    arch = re.search(r"^ARCH \?= (\S+)$", text, re.M).group(1)
    return re.search(r"^FLAGS = (.+)$", text, re.M).group(1).replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def dev():
    subprocess.check_call(["make", "-C", str(HERE)], stdout=subprocess.DEVNULL)      # up to date when it travelled with the snapshot
    if "torch" not in sys.modules:          # one HIP runtime per process: the one of the PyTorch wheel, as the package itself does
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    d = C.CDLL(str(HERE / "libdblchaindev.so"))
    assert d.dcd_chain_op_count() == len(dcc.OPS)
    return d


@pytest.fixture(scope="module")
def eg():
    import elastic_elgamal_amd as m

    return m


@pytest.fixture(scope="module")
def ctx(eg):
    c = eg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pk(golden):
    import base64

    s = golden["public_key_b64"]
    return base64.urlsafe_b64decode(s + "=" * (-len(s) % 4))


def test_flags_are_the_products():
    flags = _flags(HERE / "Makefile")
    assert flags == _flags(CSRC / "Makefile") == ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
    src = (HERE / "dblchaindev.hip").read_text() + (HERE / "chain_ops.cuh").read_text() + (HERE / "Makefile").read_text()
    assert "EG_NO_" not in src and "EG_BOUNDCHECK" not in src and "-D" not in (HERE / "Makefile").read_text()


@pytest.mark.parametrize("name", list(dcc.OPS))
def test_records_on_the_device(dev, prog, tmp_path, name):  # noqa: F811
    b = dcc.batch(name)
    assert len(b) > 256 and len(b) % 64 != 0               # several blocks and a partial last wavefront, one launch
    host = run_records(prog, tmp_path, b)                  # first: the bound-check build admits every case
    out = np.full_like(b.inp, 0xA5A5A5A5)
    step = C.c_int(0)
    status = dev.dcd_chain_ops(C.c_int(b.op), C.c_int(len(b)), b.inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_int(256),
                               C.byref(step))
    assert status == 0, f"{name}: HIP status {status} at step {step.value}"
    b.check(out)
    diff = np.nonzero((out != host).any(axis=1))[0]
    assert diff.size == 0, (name, "device and host build differ in cases", diff[:8].tolist(), [b.names[i] for i in diff[:8]])


@pytest.mark.parametrize("teeth", [5, 6])
def test_comb_product_on_the_device(dev, oracle, teeth):
    """ge_teeth_mul (sign on the accumulator, fused doubling; the table built with the fused doubling too) for every scalar of the
    list, one lane each, against the oracle's [k]P"""
    sc = [k for _, k in dcc.comb_scalars()]
    p = oracle.point_mul_generator((2**40 + 12345).to_bytes(32, "little"))
    scal = np.frombuffer(dcc.scalar_bytes(sc), dtype=np.uint32).copy()
    point = np.frombuffer(p, dtype=np.uint32).copy()
    out = np.zeros(8 * len(sc), dtype=np.uint32)
    step = C.c_int(0)
    status = dev.dcd_comb(C.c_int(teeth), C.c_int(len(sc)), scal.ctypes.data_as(C.c_void_p), point.ctypes.data_as(C.c_void_p),
                          out.ctypes.data_as(C.c_void_p), C.byref(step))
    assert status == 0, f"HIP status {status} at step {step.value}"
    raw, zero = out.tobytes(), bytes(32)
    for i, k in enumerate(sc):
        assert raw[32 * i :][:32] == oracle.point_double_mul_generator((k % L).to_bytes(32, "little"), p, zero), (teeth, hex(k))


def test_double_mul_generator_through_the_product(eg, ctx, oracle):
    """[k]P + [r]G for k and r over the scalar list (and the fixed comb's zero-digit scalars as r), P = identity, G and 8 random
    points: about 300 operations in one call, byte for byte against the oracle"""
    import torch

    rnd = random.Random("dbl-chain-double-mul")
    ks = [k for _, k in dcc.comb_scalars()]                  # 2^253 - 1 goes to the device as it is: both recodings take scalars < 2^254
    rs = [k for _, k in dcc.fixed_scalars()] + ks
    g = oracle.const_bytes(4)
    points = [bytes(32), g] + [oracle.point_mul_generator(rnd.randrange(L).to_bytes(32, "little")) for _ in range(8)]
    n = 300
    assert len(ks) >= 200 and len(rs) >= n - len(ks)
    k = [ks[i % len(ks)] for i in range(n)]
    r = [rs[(7 * i) % len(rs)] for i in range(n)]            # 7 is coprime to the list's length: every r occurs
    assert len(rs) % 7 != 0 and {x for x in r} >= set(rs[:27])
    pts = [points[i % len(points)] for i in range(n)]
    dev = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    dk, dr, dp = dev(dcc.scalar_bytes(k)), dev(dcc.scalar_bytes(r)), dev(b"".join(pts))
    do = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    dok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    eg.Ristretto(ctx).vartime_multi_mul_device(n, 1, dk.data_ptr(), dp.data_ptr(), do.data_ptr(), d_r=dr.data_ptr(), d_ok=dok.data_ptr())
    ctx.synchronize()
    out = bytes(do.cpu().numpy())
    assert dok.cpu().tolist() == [1] * n
    for i in range(n):
        want = oracle.point_double_mul_generator((k[i] % L).to_bytes(32, "little"), pts[i], (r[i] % L).to_bytes(32, "little"))
        assert out[32 * i :][:32] == want, (i, hex(k[i]), hex(r[i]))


@pytest.mark.parametrize("n_ballots", [1, 63, 300])
def test_single_choice_batches(eg, ctx, oracle, pk, n_ballots):
    """5 x 51 comb: verdict words and tally identical to the oracle's, one ballot of the batch tampered"""
    op = oracle.ChoiceParams(pk, 5, True)
    ballots = bytearray(op.generate_batch(77, 0, n_ballots))
    bad = n_ballots // 2
    ballots[bad * op.ballot_size + 320 + 32 * 3] ^= 1             # a response bit
    ballots = bytes(ballots)
    want = op.verify_batch(ballots)
    got, tally = eg.ChoiceParams(ctx, pk, 5, True).verify_batch(ballots)
    assert got == want and [i for i, s in enumerate(want) if s != 0] == [bad]
    assert tally == op.tally(ballots, want)


def test_multi_choice_and_qv_batches(eg, ctx, oracle, pk):
    """a 3-of-16 batch and a QV(5, 20) batch of 63, one ballot tampered in each: the other comb shape runs the new doubling too"""
    op = oracle.ChoiceParams(pk, 16, False)
    ballots = bytearray(op.generate_batch(5, 0, 63, n_selected=3))
    ballots[31 * op.ballot_size + 1024 + 32 * 5] ^= 1
    ballots = bytes(ballots)
    want = op.verify_batch(ballots)
    got, tally = eg.ChoiceParams(ctx, pk, 16, False).verify_batch(ballots)
    assert got == want and [i for i, s in enumerate(want) if s != 0] == [31]
    assert tally == op.tally(ballots, want)
    oq = oracle.QvParams(pk, 5, 20)
    ballots = bytearray(oq.generate_batch(9, 0, 63))
    ballots[31 * oq.ballot_size + oq.ballot_size - 32] ^= 1       # the sum response
    ballots = bytes(ballots)
    want = oq.verify_batch(ballots)
    got, tally = eg.QuadraticVotingParams(ctx, pk, 5, 20).verify_batch(ballots)
    assert got == want and [i for i, s in enumerate(want) if s != 0] == [31]
    assert tally == oq.tally(ballots, want)
