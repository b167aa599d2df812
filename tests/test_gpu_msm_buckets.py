"""The bucket method of Group::vartime_multi_mul (elastic_elgamal_amd/csrc/pippenger.cuh) at its production sizes, against the exact
reference of tests/msm_cases.py: every point has a known log, so the expected encoding is [(sum_t k_t x_t + r) mod l]G.

Points are generated on the GPU (mul_generator) from a pool of 2^16 logs and checked against the oracle before any product uses them.

Matrix (MATRIX in tests/msm_cases.py; "forced" = a context with EG_MSM_BUCKET_MIN=4096, "default" = the shipped switch at 2^20):

    case            context   terms          c  levels  mode    entries
    c12_random      forced    2^17           12   3     random  device
    c13_random      forced    2^17 + 1       13   3     random  device
    c13_digits      forced    2^17 + 1       13   3     digits  device
    c14_random      forced    2^18 + 1       14   3     random  device
    c14_digits      forced    2^18 + 1       14   3     digits  device
    c15_random      forced    2^19 + 1       15   4     random  host, device, prepared
    c15_equal       forced    2^19 + 1       15   4     equal   host, device, prepared
    c15_digits      forced    2^19 + 1       15   4     digits  device
    c15_sparse      forced    2^19 + 1       15   4     sparse  device
    c15_zero        forced    2^19 + 1       15   4     zero    host, device
    c15_pairs       forced    2^19 + 1       15   4     pairs   host, device
    c15_cancel      forced    2^19 + 1       15   4     cancel  host, device
    c15_bad         forced    2^19 + 1       15   4     bad     host, device
    c15_two         forced    2 x (2^19 + 1) 15   4     equal + random in one call: host, device
    straus_last     default   2^20 - 1       (Straus)   random  device
    bucket_first    default   2^20           15   4     random  device, prepared
    bucket_ragged   default   2^20 + 255     15   4     random  device
    advertised      default   2^22           15   4     random  device, prepared
    maximum         default   2^24           15   4     random  device

The host entry has no generator term; the device and prepared entries add [r]G, and the device entry's d_ok must say whether every
point decoded.  The zero, pairs and cancel cases must give 32 zero bytes without r.  The c15_pairs case sums to the identity in every
bucket, so it does not depend on the window weights: it guards the bucket lists and the level sums, not k_pip_window.  Two cases guard
no seeded kernel fault: straus_last checks that the size just below the switch still runs (and is right) on the Straus path, and
c15_zero that a problem whose buckets are all empty (no pieces at any level, every window sum the identity) gives the identity.
"""
import os

import numpy as np
import pytest

import msm_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eg():
    import elastic_elgamal_amd as m

    return m


@pytest.fixture(scope="module")
def groups(eg):
    saved = os.environ.pop("EG_MSM_BUCKET_MIN", None)
    try:
        os.environ["EG_MSM_BUCKET_MIN"] = str(mc.FORCED_BUCKET_MIN)   # read once, by eg_init
        forced = eg.Context(0)
        os.environ.pop("EG_MSM_BUCKET_MIN")
        default = eg.Context(0)
    finally:
        if saved is not None:
            os.environ["EG_MSM_BUCKET_MIN"] = saved
    yield {"forced": (forced, eg.Ristretto(forced)), "default": (default, eg.Ristretto(default))}
    forced.close()
    default.close()


@pytest.fixture(scope="module")
def pool():
    return mc.make_pool()


@pytest.fixture(scope="module")
def pool_dev(groups, pool, eg):
    """The pool's encodings (generated on the GPU, a sample checked against the oracle) and its prepared points, on the device."""
    import torch

    ctx, grp = groups["default"]
    enc = grp.mul_generator(b"".join(mc.sc(x) for x in pool.logs))
    n = len(pool)
    rnd = np.random.default_rng(7)
    sample = sorted({0, 1, 2, pool.half, pool.half + 1, n - 1} | set(rnd.choice(n, 1024, replace=False).tolist()))
    for j in sample:
        assert enc[32 * j : 32 * j + 32] == pool.encoding(j), j
    d_enc = torch.frombuffer(bytearray(enc), dtype=torch.uint8).cuda().view(n, 32)
    prep = torch.zeros((n, eg.prepared_point_size()), dtype=torch.uint8, device="cuda")
    pok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    grp.prepare_points_device(n, d_enc.data_ptr(), prep.data_ptr(), d_ok=pok.data_ptr())
    ctx.synchronize()
    assert int(pok.min()) == 1
    return d_enc, prep


@pytest.mark.parametrize("spec", mc.MATRIX, ids=lambda s: s.name)
def test_bucket_method_against_exact_reference(groups, pool, pool_dev, spec):
    import torch

    ctx, grp = groups[spec.ctx]
    d_enc, d_prep = pool_dev
    cases = mc.build(spec.mode, spec.terms, pool, spec.seed)
    m, terms = len(cases), spec.terms
    want = [case.expected(pool) for case in cases]
    want_r = [case.expected(pool, with_r=True) for case in cases]
    ok_want = [0 if case.bad else 1 for case in cases]
    if spec.mode in ("zero", "pairs", "cancel"):
        assert want == [bytes(32)] * m
    idx = torch.from_numpy(np.concatenate([case.idx for case in cases])).cuda()
    ds = torch.from_numpy(np.concatenate([case.scalars for case in cases])).cuda()
    dp = d_enc[idx]
    for i, case in enumerate(cases):
        for t in case.bad:
            dp[i * terms + t] = 0xFF
    dr = torch.from_numpy(np.concatenate([mc._from_ints([case.r]) for case in cases])).cuda()
    need = grp.msm_scratch_bytes(m, terms)
    assert need > 0
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    do = torch.zeros((m, 32), dtype=torch.uint8, device="cuda")

    if "host" in spec.entries:
        out, ok = grp.vartime_multi_mul(terms, bytes(ds.cpu().numpy()), bytes(dp.cpu().numpy()))
        assert list(ok) == ok_want, spec.name
        for i in range(m):
            assert out[32 * i : 32 * i + 32] == want[i], (spec.name, "host", i)
    if "device" in spec.entries:
        dok = torch.full((m,), 7, dtype=torch.uint8, device="cuda")
        grp.vartime_multi_mul_device(m, terms, ds.data_ptr(), dp.data_ptr(), do.data_ptr(), d_r=dr.data_ptr(), d_scratch=scratch.data_ptr(),
                                     d_ok=dok.data_ptr())
        ctx.synchronize()
        assert dok.cpu().tolist() == ok_want, spec.name
        out = bytes(do.cpu().numpy())
        for i in range(m):
            assert out[32 * i : 32 * i + 32] == want_r[i], (spec.name, "device", i)
    if "prepared" in spec.entries:
        assert not any(case.bad for case in cases)
        prep = d_prep[idx]
        do.zero_()
        grp.vartime_multi_mul_prepared_device(m, terms, ds.data_ptr(), prep.data_ptr(), do.data_ptr(), d_r=dr.data_ptr(),
                                              d_scratch=scratch.data_ptr())
        ctx.synchronize()
        out = bytes(do.cpu().numpy())
        for i in range(m):
            assert out[32 * i : 32 * i + 32] == want_r[i], (spec.name, "prepared", i)
