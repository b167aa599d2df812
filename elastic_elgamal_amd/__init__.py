"""elastic_elgamal_amd -- MI355X (gfx950) batch verifier for slowli/elastic-elgamal ballots.

Python host-side mirror of the reference interface for the ballot-verification hot path, bound with
ctypes to the C ABI of ``libeg_hip.so`` (``include/eg_hip.h``).  Names follow the reference:

* :class:`Ristretto`              -- the ``Group`` backend (src/group/ristretto.rs), batched
* :class:`ChoiceParams`           -- ``ChoiceParams::single / ::multi`` (src/app/choice.rs:132-196) with
  ``verify_batch`` = ``EncryptedChoice::verify`` for every ballot (choice.rs:358-380) + the homomorphic tally
  of examples/voting.rs:199-203
* :class:`QuadraticVotingParams`  -- ``QuadraticVotingParams::new`` (src/app/quadratic_voting.rs:63-76) with
  ``verify_batch`` = ``QuadraticVotingBallot::verify`` (quadratic_voting.rs:291-329)

There is NO CPU path in this package: if the HIP library is missing or no gfx950 device is usable, importing
works but creating a :class:`Context` raises.  (The CPU oracle lives under ``oracle/`` and is test-only.)
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

__all__ = [
    "Context", "Ristretto", "Ed25519", "VoterRoll", "ReceiptLog", "ChoiceParams", "QuadraticVotingParams", "PublicKeyVerifier", "DecryptionShareVerifier", "SumOfSquaresVerifier", "EgError", "library_path", "build",
    "STATUS_NAMES", "status_kind", "status_detail", "pack_json", "JsonPacker", "PACK_RESHAPE", "verify_json_multi", "json_stream_multi",
]

_PKG = Path(__file__).resolve().parent
_LIB = Path(os.environ.get("EG_LIB", str(_PKG / "libeg_hip.so")))   # EG_LIB: alternate build for A/B measurements

OK, BAD_SCALAR, BAD_POINT, OPTIONS_LEN, SUM_CHALLENGE, RANGE_LEN, RANGE_CHALLENGE = range(7)
QV_VARIANT_LEN, QV_VARIANT_CHALLENGE, QV_CREDIT_RANGE_LEN, QV_CREDIT_RANGE_CHALLENGE = 7, 8, 9, 10
QV_CREDIT_EQUIV_LEN, QV_CREDIT_EQUIV_CHALLENGE = 11, 12
MALFORMED = 13
STATUS_NAMES = {
    0: "Ok", 1: "BadScalar", 2: "BadPoint", 3: "OptionsLenMismatch", 4: "Sum(ChallengeMismatch)",
    5: "Range(LenMismatch)", 6: "Range(ChallengeMismatch)", 7: "Variant(LenMismatch)", 8: "Variant(ChallengeMismatch)",
    9: "CreditRange(LenMismatch)", 10: "CreditRange(ChallengeMismatch)", 11: "CreditEquivalence(LenMismatch)",
    12: "CreditEquivalence(ChallengeMismatch)", 13: "Malformed", 14: "Duplicate",
    15: "BadSignature", 16: "Superseded",
}


def status_kind(s: int) -> int:
    return s & 0xFF


def status_detail(s: int) -> int:
    return s >> 8


class EgError(RuntimeError):
    pass


def effective_cores() -> int:
    """Hardware threads this process may actually use (affinity mask and cgroup CPU quota): the default size of the parser's thread pool.
    os.cpu_count() is the machine's - 256 on a box that grants 16 - and oversubscribing the pool 16-fold costs an order of magnitude."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = Path("/sys/fs/cgroup/cpu.max").read_text().split()
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period) + 0.5)))
    except Exception:
        pass
    return n


def library_path() -> Path:
    return _LIB


def build(verbose: bool = False) -> Path:
    """Compile csrc/eg_hip.hip for gfx950 with hipcc into the in-tree libeg_hip.so (no GPU needed)."""
    import subprocess

    deps = list((_PKG / "csrc").glob("*.hip")) + list((_PKG / "csrc").glob("*.cuh")) + list((_PKG / "csrc").glob("*.h*"))
    deps.append(_PKG.parent / "include" / "eg_hip.h")
    if _LIB.exists() and all(d.stat().st_mtime <= _LIB.stat().st_mtime for d in deps):
        return _LIB
    cmd = ["make", "-C", str(_PKG / "csrc"), "-j4"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return _LIB


_lib = None
_RELEASE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t)      # eg_json_release_fn
# blocks given back by the library to feed_owned_ptr callers: counted by the library's own eg_json_release_count (a C function: a Python
# callback would take the interpreter lock on the stream's worker thread once per block, in competition with the feeding thread)
_released_blocks = C.c_size_t(0)


def released_blocks() -> int:
    return int(_released_blocks.value)


def _load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB.exists():
        raise EgError(
            f"{_LIB} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    # PyTorch-ROCm wheels carry their OWN libamdhip64 / HSA runtime.  Two HIP runtimes in one process do not share the device: whichever
    # loads second reports "No HIP GPUs are available".  A process that uses torch for device memory (tests, bench.py) must therefore load
    # torch's runtime first; libeg_hip.so then binds to the copy that is already there.  (A host without torch is unaffected.)
    import sys
    if "torch" not in sys.modules and not os.environ.get("EG_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(str(_LIB))
    vp, cp, sz = C.c_void_p, C.c_char_p, C.c_size_t
    sig = {
        "eg_init": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "eg_destroy": (None, [vp]),
        "eg_last_error": (cp, []),
        "eg_device_name": (C.c_int, [vp, cp, sz]),
        "eg_synchronize": (C.c_int, [vp]),
        "eg_scalar_from_wide_batch": (C.c_int, [vp, sz, cp, cp]),
        "eg_scalar_is_canonical_batch": (C.c_int, [vp, sz, cp, cp]),
        "eg_scalar_muladd_batch": (C.c_int, [vp, sz, cp, cp, cp, cp]),
        "eg_scalar_neg_batch": (C.c_int, [vp, sz, cp, cp]),
        "eg_scalar_invert_batch": (C.c_int, [vp, sz, cp, cp]),
        "eg_point_is_identity_batch": (C.c_int, [vp, sz, cp, cp, cp]),
        "eg_point_roundtrip_batch": (C.c_int, [vp, sz, cp, cp, cp]),
        "eg_point_add_batch": (C.c_int, [vp, sz, cp, cp, C.c_int, cp, cp]),
        "eg_mul_generator_batch": (C.c_int, [vp, sz, cp, cp]),
        "eg_vartime_double_mul_generator_batch": (C.c_int, [vp, sz, cp, cp, cp, cp, cp]),
        "eg_vartime_multi_mul_batch": (C.c_int, [vp, sz, sz, cp, cp, cp, cp]),
        "eg_abi_version": (C.c_int, []),
        "eg_msm_scratch_bytes_ctx": (sz, [vp, sz, sz]),
        "eg_selfbench_fmul": (C.c_int, [vp, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "eg_choice_prepare_wide_tables": (C.c_int, [vp]),
        "eg_qv_prepare_wide_tables": (C.c_int, [vp]),
        "eg_combine_shares": (C.c_int, [vp, C.c_uint64, C.c_uint64, sz, C.POINTER(C.c_uint64), cp, cp, C.POINTER(C.c_int)]),
        "eg_combine_shares_batch_scratch_bytes": (sz, [C.c_uint64, sz]),
        "eg_combine_shares_batch_device": (C.c_int, [vp, C.c_uint64, C.c_uint64, sz, vp, C.c_int, C.POINTER(C.c_uint64), vp, vp, vp, vp, vp, vp, vp,
                                                     vp, vp]),
        "eg_combine_shares_batch": (C.c_int, [vp, C.c_uint64, C.c_uint64, sz, vp, C.c_int, C.POINTER(C.c_uint64), vp, vp, vp, vp, vp, vp]),
        "eg_dlog_table_create": (C.c_int, [vp, sz, C.POINTER(C.c_uint64), C.POINTER(vp)]),
        "eg_dlog_table_destroy": (None, [vp]),
        "eg_dlog_table_get": (C.c_int, [vp, sz, cp, C.POINTER(C.c_uint64), cp]),
        "eg_dlog_solver_create": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
        "eg_dlog_solver_destroy": (None, [vp]),
        "eg_dlog_solver_solve": (C.c_int, [vp, sz, cp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), cp]),
        "eg_dlog_solver_max_span": (C.c_uint64, [vp, sz]),
        "eg_dlog_solver_table_bytes": (sz, [vp]),
        "eg_vartime_multi_mul_batch_device": (C.c_int, [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]),
        "eg_prepared_point_size": (sz, []),
        "eg_points_prepare_device": (C.c_int, [vp, sz, vp, vp, vp, vp]),
        "eg_vartime_multi_mul_prepared_batch_device": (C.c_int, [vp, sz, sz, vp, vp, vp, vp, vp, vp]),
        "eg_choice_params_create": (C.c_int, [vp, cp, C.c_int, C.c_int, C.POINTER(vp)]),
        "eg_choice_params_destroy": (None, [vp]),
        "eg_choice_ballot_size": (sz, [C.c_int, C.c_int]),
        "eg_verify_choice_batch": (C.c_int, [vp, sz, vp, vp, vp]),
        "eg_verify_choice_batch_device": (C.c_int, [vp, sz, vp, vp, vp]),
        "eg_choice_tally_reset": (C.c_int, [vp]),
        "eg_choice_tally_add": (C.c_int, [vp, cp]),
        "eg_qv_tally_add": (C.c_int, [vp, cp]),
        "eg_choice_tally_encode": (C.c_int, [vp, cp]),
        "eg_qv_params_create": (C.c_int, [vp, cp, C.c_int, C.c_uint64, C.POINTER(vp)]),
        "eg_qv_params_destroy": (None, [vp]),
        "eg_qv_ballot_size": (sz, [vp]),
        "eg_verify_qv_batch": (C.c_int, [vp, sz, vp, vp, vp]),
        "eg_verify_qv_batch_device": (C.c_int, [vp, sz, vp, vp, vp]),
        "eg_verify_choice_small": (C.c_int, [vp, sz, vp, vp, vp]),
        "eg_verify_choice_small_device": (C.c_int, [vp, sz, vp, vp, vp]),
        "eg_verify_qv_small": (C.c_int, [vp, sz, vp, vp, vp]),
        "eg_verify_qv_small_device": (C.c_int, [vp, sz, vp, vp, vp]),
        "eg_qv_tally_reset": (C.c_int, [vp]),
        "eg_qv_tally_encode": (C.c_int, [vp, cp]),
        "eg_verify_choice_batch_multi": (C.c_int, [C.POINTER(vp), C.c_int, sz, vp, vp, vp]),
        "eg_verify_qv_batch_multi": (C.c_int, [C.POINTER(vp), C.c_int, sz, vp, vp, vp]),
        "eg_verify_choice_batch_multi_device": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(sz), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]),
        "eg_verify_qv_batch_multi_device": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(sz), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]),
        "eg_choice_tally_encode_multi": (C.c_int, [C.POINTER(vp), C.c_int, cp]),
        "eg_qv_tally_encode_multi": (C.c_int, [C.POINTER(vp), C.c_int, cp]),
        "eg_choice_tally_reset_async": (C.c_int, [vp, vp]),
        "eg_choice_tally_encode_device": (C.c_int, [vp, vp, vp]),
        "eg_qv_tally_reset_async": (C.c_int, [vp, vp]),
        "eg_qv_tally_encode_device": (C.c_int, [vp, vp, vp]),
        "eg_points_sum_device": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp]),
        "eg_choice_tally_grouped_scratch_bytes": (sz, [vp, sz, C.c_uint32]),
        "eg_choice_tally_grouped_device": (C.c_int, [vp, sz, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp]),
        "eg_choice_tally_grouped": (C.c_int, [vp, sz, vp, vp, vp, C.c_uint32, vp, vp]),
        "eg_qv_tally_grouped_scratch_bytes": (sz, [vp, sz, C.c_uint32]),
        "eg_qv_tally_grouped_device": (C.c_int, [vp, sz, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp]),
        "eg_qv_tally_grouped": (C.c_int, [vp, sz, vp, vp, vp, C.c_uint32, vp, vp]),
        "eg_choice_tally_weighted_scratch_bytes": (sz, [vp, sz, C.c_uint32]),
        "eg_choice_tally_weighted_device": (C.c_int, [vp, sz, vp, vp, vp, C.c_int, vp, C.c_uint32, vp, vp, vp, vp, vp, vp]),
        "eg_choice_tally_weighted": (C.c_int, [vp, sz, vp, vp, vp, C.c_int, vp, C.c_uint32, vp, vp, vp]),
        "eg_qv_tally_weighted_scratch_bytes": (sz, [vp, sz, C.c_uint32]),
        "eg_qv_tally_weighted_device": (C.c_int, [vp, sz, vp, vp, vp, C.c_int, vp, C.c_uint32, vp, vp, vp, vp, vp, vp]),
        "eg_qv_tally_weighted": (C.c_int, [vp, sz, vp, vp, vp, C.c_int, vp, C.c_uint32, vp, vp, vp]),
        "eg_choice_weed_scratch_bytes": (sz, [vp, sz, sz]),
        "eg_choice_weed_device": (C.c_int, [vp, sz, vp, vp, sz, vp, sz, C.c_uint64, vp, vp, vp, vp, vp, vp]),
        "eg_choice_weed": (C.c_int, [vp, sz, vp, vp, sz, vp, vp, vp, vp, C.POINTER(sz)]),
        "eg_qv_weed_scratch_bytes": (sz, [vp, sz, sz]),
        "eg_qv_weed_device": (C.c_int, [vp, sz, vp, vp, sz, vp, sz, C.c_uint64, vp, vp, vp, vp, vp, vp]),
        "eg_qv_weed": (C.c_int, [vp, sz, vp, vp, sz, vp, vp, vp, vp, C.POINTER(sz)]),
        "eg_weed_index_bytes": (sz, [sz]),
        "eg_weed_index_build_device": (C.c_int, [vp, sz, vp, sz, C.c_uint64, vp, vp, vp]),
        "eg_weed_index_find_device": (C.c_int, [vp, sz, vp, sz, vp, sz, vp, C.c_uint64, vp, vp]),
        "eg_choice_weed_indexed_scratch_bytes": (sz, [vp, sz]),
        "eg_choice_weed_indexed_device": (C.c_int, [vp, sz, vp, vp, sz, vp, sz, vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp, vp]),
        "eg_qv_weed_indexed_scratch_bytes": (sz, [vp, sz]),
        "eg_qv_weed_indexed_device": (C.c_int, [vp, sz, vp, vp, sz, vp, sz, vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp, vp]),
        "eg_choice_open_check_scratch_bytes": (sz, [vp, sz]),
        "eg_choice_open_check_device": (C.c_int, [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]),
        "eg_choice_open_check": (C.c_int, [vp, sz, vp, vp, vp, vp, vp, vp]),
        "eg_qv_open_check_scratch_bytes": (sz, [vp, sz]),
        "eg_qv_open_check_device": (C.c_int, [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]),
        "eg_qv_open_check": (C.c_int, [vp, sz, vp, vp, vp, vp, vp, vp]),
        "eg_choice_open_batch_device": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_int, C.c_uint64, vp, vp, vp, vp]),
        "eg_choice_open_batch": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_int, C.c_uint64, vp, vp, vp]),
        "eg_qv_open_batch_device": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_uint64, vp, vp, vp, vp]),
        "eg_qv_open_batch": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_uint64, vp, vp, vp]),
        "eg_ed25519_verify_scratch_bytes": (sz, [vp, sz]),
        "eg_ed25519_verify_device": (C.c_int, [vp, sz, vp, sz, sz, cp, sz, vp, sz, vp, vp, vp, vp, vp, sz, vp]),
        "eg_ed25519_verify_batch": (C.c_int, [vp, sz, cp, sz, sz, cp, sz, cp, sz, vp, cp, vp, vp]),
        "eg_ed25519_keypair_batch": (C.c_int, [vp, sz, cp, cp]),
        "eg_ed25519_keypair_batch_device": (C.c_int, [vp, sz, vp, vp, vp]),
        "eg_ed25519_sign_batch": (C.c_int, [vp, sz, cp, cp, sz, sz, cp, sz, cp]),
        "eg_ed25519_sign_batch_device": (C.c_int, [vp, sz, vp, vp, sz, sz, vp, sz, vp, vp]),
        "eg_sha512_batch": (C.c_int, [vp, sz, cp, sz, sz, cp, sz, cp]),
        "eg_sha512_batch_device": (C.c_int, [vp, sz, vp, sz, sz, vp, sz, vp, vp]),
        "eg_roll_cast_scratch_bytes": (sz, [vp, sz, sz]),
        "eg_roll_cast_device": (C.c_int, [vp, sz, vp, vp, C.c_uint64, C.c_int, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "eg_roll_cast": (C.c_int, [vp, sz, vp, vp, C.c_uint64, C.c_int, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "eg_roll_check_device": (C.c_int, [vp, sz, vp, vp, C.c_uint64, C.c_int, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]),
        "eg_roll_check": (C.c_int, [vp, sz, vp, vp, C.c_uint64, C.c_int, vp, sz, vp, vp, vp, vp, vp, vp, vp]),
        "eg_merkle_depth": (C.c_int, [C.c_uint64]),
        "eg_merkle_nodes_bytes": (sz, [C.c_uint64]),
        "eg_merkle_level": (C.c_int, [C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "eg_merkle_leaves_scratch_bytes": (sz, [sz]),
        "eg_merkle_tree_scratch_bytes": (sz, [C.c_uint64]),
        "eg_merkle_leaves_device": (C.c_int, [vp, sz, vp, sz, sz, cp, sz, vp, sz, sz, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp, vp, sz, vp]),
        "eg_merkle_leaves": (C.c_int, [vp, sz, cp, sz, sz, cp, sz, cp, sz, sz, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp]),
        "eg_merkle_tree_device": (C.c_int, [vp, C.c_uint64, vp, vp, vp, vp, sz, vp]),
        "eg_merkle_tree": (C.c_int, [vp, C.c_uint64, cp, vp, vp]),
        "eg_merkle_paths_device": (C.c_int, [vp, sz, vp, C.c_uint64, vp, vp, vp, vp, vp]),
        "eg_merkle_paths": (C.c_int, [vp, sz, vp, C.c_uint64, cp, cp, vp, vp]),
        "eg_merkle_check_device": (C.c_int, [vp, sz, vp, vp, vp, sz, vp, C.c_uint64, vp, vp, vp, vp]),
        "eg_merkle_check": (C.c_int, [vp, sz, vp, cp, cp, sz, vp, C.c_uint64, cp, vp, vp]),
        "eg_merkle_consistency_len": (C.c_uint32, [C.c_uint64, C.c_uint64]),
        "eg_merkle_heads_device": (C.c_int, [vp, sz, vp, C.c_uint64, vp, vp, vp, vp, vp]),
        "eg_merkle_heads": (C.c_int, [vp, sz, vp, C.c_uint64, cp, cp, vp, vp]),
        "eg_merkle_consistency_device": (C.c_int, [vp, sz, vp, C.c_uint64, vp, vp, vp, vp, vp]),
        "eg_merkle_consistency": (C.c_int, [vp, sz, vp, C.c_uint64, cp, cp, vp, vp]),
        "eg_merkle_consistency_check_device": (C.c_int, [vp, sz, vp, vp, vp, sz, vp, C.c_uint64, vp, vp, vp, vp]),
        "eg_merkle_consistency_check": (C.c_int, [vp, sz, vp, cp, cp, sz, vp, C.c_uint64, cp, vp, vp]),
        "eg_merkle_grow_device": (C.c_int, [vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp]),
        "eg_merkle_grow": (C.c_int, [vp, C.c_uint64, cp, C.c_uint64, cp, vp, vp]),
        "eg_shuffle_key_bytes": (sz, [C.c_uint64]),
        "eg_shuffle_proof_bytes": (sz, [C.c_uint64]),
        "eg_shuffle_key_derive_device": (C.c_int, [vp, cp, sz, C.c_uint64, vp, vp, vp]),
        "eg_shuffle_key_derive": (C.c_int, [vp, cp, sz, C.c_uint64, vp]),
        "eg_shuffle_verify_scratch_bytes": (sz, [vp, C.c_uint64]),
        "eg_shuffle_verify_device": (C.c_int, [vp, C.c_uint64, vp, vp, cp, cp, sz, vp, C.c_uint64, vp, vp, vp, vp, vp, sz, vp]),
        "eg_shuffle_verify": (C.c_int, [vp, C.c_uint64, cp, cp, cp, cp, sz, cp, C.c_uint64, cp, vp, vp, vp]),
        "eg_proof_params_create": (C.c_int, [vp, cp, C.c_int, C.c_uint64, C.POINTER(vp)]),
        "eg_share_params_create": (C.c_int, [vp, cp, C.c_uint64, C.c_uint64, C.c_uint64, cp, C.POINTER(vp)]),
        "eg_proof_params_destroy": (None, [vp]),
        "eg_proof_item_size": (sz, [vp]),
        "eg_verify_proof_batch": (C.c_int, [vp, sz, vp, vp]),
        "eg_verify_proof_batch_device": (C.c_int, [vp, sz, vp, vp, vp]),
        "eg_choice_encrypt_batch": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_int, cp]),
        "eg_choice_encrypt_batch_device": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_int, vp, vp]),
        "eg_qv_encrypt_batch_device": (C.c_int, [vp, C.c_uint64, sz, sz, vp, vp]),
        "eg_choice_encrypt_selected_batch": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_uint64, vp, cp]),
        "eg_choice_encrypt_selected_batch_device": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_uint64, vp, vp, vp]),
        "eg_qv_encrypt_votes_batch": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_uint64, vp, cp]),
        "eg_qv_encrypt_votes_batch_device": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_uint64, vp, vp, vp]),
        "eg_sumsq_params_create": (C.c_int, [vp, cp, C.c_int, cp, sz, C.POINTER(vp)]),
        "eg_commit_equiv_params_create": (C.c_int, [vp, cp, cp, cp, sz, C.POINTER(vp)]),
        "eg_commit_equiv_prove_batch": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_uint64, vp, vp, vp]),
        "eg_commit_equiv_prove_batch_device": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_uint64, vp, vp, vp, vp]),
        "eg_proof_prove_input_size": (sz, [vp]),
        "eg_proof_prove_batch": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_uint64, vp, vp]),
        "eg_proof_prove_batch_device": (C.c_int, [vp, C.c_uint64, sz, sz, C.c_uint64, vp, vp, vp]),
        "eg_share_prove_batch": (C.c_int, [vp, cp, C.c_uint64, sz, sz, C.c_uint64, vp, vp, vp]),
        "eg_share_prove_batch_device": (C.c_int, [vp, cp, C.c_uint64, sz, sz, C.c_uint64, vp, vp, vp, vp]),
        "eg_merlin_challenge_batch": (C.c_int, [vp, sz, cp, sz, cp, sz, cp, sz, cp, sz, cp, sz]),
        "eg_choice_pack_json": (C.c_int, [C.c_int, C.c_int, cp, sz, C.c_int, sz, vp, vp, C.POINTER(sz)]),
        "eg_qv_pack_json": (C.c_int, [C.c_int, C.c_uint64, cp, sz, C.c_int, sz, vp, vp, C.POINTER(sz)]),
        "eg_qv_ballot_size_for": (sz, [C.c_int, C.c_uint64]),
        "eg_verify_choice_json": (C.c_int, [vp, vp, sz, C.c_int, sz, vp, C.POINTER(sz), vp]),
        "eg_verify_qv_json": (C.c_int, [vp, vp, sz, C.c_int, sz, vp, C.POINTER(sz), vp]),
        "eg_verify_choice_json_multi": (C.c_int, [C.POINTER(vp), C.c_int, vp, sz, C.c_int, sz, vp, C.POINTER(sz), vp]),
        "eg_verify_qv_json_multi": (C.c_int, [C.POINTER(vp), C.c_int, vp, sz, C.c_int, sz, vp, C.POINTER(sz), vp]),
        "eg_verify_choice_json_begin_multi": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(vp)]),
        "eg_verify_qv_json_begin_multi": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(vp)]),
        "eg_verify_choice_json_begin": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
        "eg_verify_qv_json_begin": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
        "eg_verify_json_feed": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
        "eg_verify_json_feed_owned": (C.c_int, [vp, vp, sz, vp, vp, C.POINTER(sz)]),
        "eg_json_release_count": (None, [vp, vp, sz]),
        "eg_verify_json_take": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
        "eg_verify_json_end": (C.c_int, [vp, vp, sz, C.POINTER(sz), C.POINTER(sz), vp]),
        "eg_verify_json_abort": (None, [vp]),
        "eg_range_decomposition": (C.c_int, [C.c_uint64, cp, sz]),
        "eg_plan_describe": (C.c_int, [C.c_int, C.c_int, C.c_uint64, cp, sz]),
        "eg_profile_enable": (C.c_int, [vp, C.c_int]),
        "eg_profile_read": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
        "eg_profile_read_tables": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "eg_selfcheck_generator_table": (C.c_int, [vp, C.c_int, sz, C.c_uint64, C.POINTER(C.c_uint64)]),
        "eg_comb_table_bits": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    }
    for name, (res, args) in sig.items():
        if "EG_LIB" in os.environ and not hasattr(lib, name):
            continue             # an alternate (older) build selected for an A/B measurement may lack the newest entry points
        fn = getattr(lib, name)  # raises AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    if "EG_LIB" not in os.environ and lib.eg_abi_version() != ABI_VERSION:
        raise EgError(f"{_LIB} speaks ABI version {lib.eg_abi_version()}, this binding expects {ABI_VERSION}: rebuild it")
    _lib = lib
    return lib


PACK_RESHAPE = 0xFFFFFFFE
ABI_VERSION = 7          # include/eg_hip.h: EG_ABI_VERSION
SMALL_BATCH_MAX = 4096   # include/eg_hip.h: EG_SMALL_BATCH_MAX, the most ballots one verify_small call takes
GROUP_NONE = 0xFFFFFFFF          # include/eg_hip.h: EG_GROUP_NONE, the group id that leaves a ballot out of every group
TALLY_GROUPS_MAX = 1 << 24       # include/eg_hip.h: EG_TALLY_GROUPS_MAX
ST_DUPLICATE = 14                # include/eg_hip.h: EG_ST_DUPLICATE, what weed() writes into status_out for a flagged ballot
DUP_NONE = 0xFFFFFFFF            # include/eg_hip.h: EG_DUP_NONE
DUP_PRIOR = 0xFFFFFFFE           # include/eg_hip.h: EG_DUP_PRIOR, a ballot that repeats a ciphertext of the board
WEED_KEYS_MAX = 1 << 30          # include/eg_hip.h: EG_WEED_KEYS_MAX
ST_BAD_SIGNATURE = 15            # include/eg_hip.h: EG_ST_BAD_SIGNATURE, what Ed25519.verify writes; the detail is one of ED25519_*
ED25519_BAD_S, ED25519_BAD_KEY, ED25519_SMALL_ORDER, ED25519_MISMATCH, ED25519_BAD_INDEX = 1, 2, 3, 4, 5
ST_SUPERSEDED = 16               # include/eg_hip.h: EG_ST_SUPERSEDED, what VoterRoll writes into status_out; the detail is one of ROLL_*
ROLL_FIRST, ROLL_LAST = 1, 2     # include/eg_hip.h: EG_ROLL_FIRST / EG_ROLL_LAST, the policy of a roll
ROLL_SUPERSEDED, ROLL_OFF_ROLL, ROLL_NOT_CAST = 1, 2, 3
SEQ_NONE = (1 << 64) - 1         # include/eg_hip.h: EG_SEQ_NONE
ROLL_KEYS_MAX = 1 << 31          # include/eg_hip.h: EG_ROLL_KEYS_MAX
ST_BAD_OPENING = 17              # include/eg_hip.h: EG_ST_BAD_OPENING, what open_check writes; the detail is open_detail(slot, check)
OPEN_BAD_SCALAR, OPEN_R, OPEN_B = 1, 2, 3    # include/eg_hip.h: EG_OPEN_*, the check of an opening that failed
OPEN_ITEMS_MAX = 1 << 31         # include/eg_hip.h: EG_OPEN_ITEMS_MAX


def open_detail(slot: int, check: int) -> int:
    """EG_OPEN_DETAIL: the detail of a status word of kind ST_BAD_OPENING; slot = detail >> 2, check = detail & 3."""
    return slot * 4 + check


MERKLE_BAD_INDEX, MERKLE_BAD_LENGTH, MERKLE_MISMATCH = 1, 2, 3    # include/eg_hip.h: EG_MERKLE_*, the verdict of a receipt
MERKLE_MISMATCH_OLD = 4          # include/eg_hip.h: EG_MERKLE_MISMATCH_OLD, a consistency proof that does not give the old root
MERKLE_HASH_BYTES = 32           # include/eg_hip.h: EG_MERKLE_HASH_BYTES
MERKLE_LEAVES_MAX = 1 << 31      # include/eg_hip.h: EG_MERKLE_LEAVES_MAX
LEAF_NONE = (1 << 64) - 1        # include/eg_hip.h: EG_LEAF_NONE, the leaf_index of a ballot that does not participate
MERKLE_NO_PATH = 0xFFFFFFFF      # include/eg_hip.h: EG_MERKLE_NO_PATH, the path_len of an index that is not in the log
SHUFFLE_BAD_ENCODING, SHUFFLE_T1, SHUFFLE_T2, SHUFFLE_T3, SHUFFLE_T41, SHUFFLE_T42, SHUFFLE_CHAIN = 1, 2, 4, 8, 16, 32, 64   # EG_SHUFFLE_*
SHUFFLE_ROW_BAD, SHUFFLE_ROW_CHAIN = 1, 2    # include/eg_hip.h: EG_SHUFFLE_ROW_*, the bits of a row's word
SHUFFLE_ROWS_MAX = 1 << 23       # include/eg_hip.h: EG_SHUFFLE_ROWS_MAX
SHUFFLE_KEY_TRIES = 4096         # include/eg_hip.h: EG_SHUFFLE_KEY_TRIES


def pack_json(text, n_options: int, single: bool | None = None, credits: int | None = None, threads: int = 0, max_objects: int = 0):
    """Native wire ingest (csrc/wire_json.hpp; no GPU needed): ballots in serde's JSON layout (one array, or objects back to
    back) -> (packed bytes of ALL objects, status words).  Object k occupies packed[k*size:(k+1)*size] and is valid iff
    status[k] == 0; MALFORMED = does not deserialise, PACK_RESHAPE = wrong number of choices / responses (object path).
    `credits` selects QuadraticVotingBallot, otherwise EncryptedChoice with `single`."""
    lib = _load()
    data = text.encode() if isinstance(text, str) else bytes(text)
    if not threads:
        threads = effective_cores()
    size = lib.eg_qv_ballot_size_for(n_options, credits) if credits is not None else lib.eg_choice_ballot_size(n_options, int(bool(single)))
    if not size:
        raise EgError("bad election parameters")
    if not max_objects:
        # the library counts the objects itself (max_objects = 0: nothing is written, *n_objects says how many there are); counting a
        # key word instead would undercount texts that hold junk objects, and one voter's junk must never block the others' ballots
        n0 = sz_t(0)
        if credits is not None:
            rc = lib.eg_qv_pack_json(n_options, credits, data, len(data), threads, 0, None, None, C.byref(n0))
        else:
            rc = lib.eg_choice_pack_json(n_options, int(bool(single)), data, len(data), threads, 0, None, None, C.byref(n0))
        if rc != 0 and n0.value == 0:
            _check(rc)
        max_objects = n0.value
    packed = C.create_string_buffer(max(max_objects * size, 1))
    status = (C.c_uint32 * max(max_objects, 1))()
    n = sz_t(0)
    if credits is not None:
        _check(lib.eg_qv_pack_json(n_options, credits, data, len(data), threads, max_objects, packed, status, C.byref(n)))
    else:
        _check(lib.eg_choice_pack_json(n_options, int(bool(single)), data, len(data), threads, max_objects, packed, status, C.byref(n)))
    return packed.raw[: n.value * size], list(status[: n.value])


sz_t = C.c_size_t


class JsonPacker:
    """The native packer with caller-owned, reusable output buffers (what a native host does): no allocation or copy per call.
    `pack(text)` returns the number of objects; `packed` (a ctypes buffer) and `status` hold the results."""

    def __init__(self, n_options: int, max_objects: int, single: bool | None = None, credits: int | None = None, threads: int = 0):
        lib = _load()
        self.n_options, self.single, self.credits, self.max_objects = n_options, single, credits, max_objects
        self.threads = threads or effective_cores()
        self.ballot_size = (lib.eg_qv_ballot_size_for(n_options, credits) if credits is not None
                            else lib.eg_choice_ballot_size(n_options, int(bool(single))))
        if not self.ballot_size:
            raise EgError("bad election parameters")
        self.packed = C.create_string_buffer(max(max_objects * self.ballot_size, 1))
        self.status = (C.c_uint32 * max(max_objects, 1))()

    def pack(self, data: bytes) -> int:
        n = sz_t(0)
        lib = _load()
        if self.credits is not None:
            _check(lib.eg_qv_pack_json(self.n_options, self.credits, data, len(data), self.threads, self.max_objects, self.packed,
                                       self.status, C.byref(n)))
        else:
            _check(lib.eg_choice_pack_json(self.n_options, int(bool(self.single)), data, len(data), self.threads, self.max_objects,
                                           self.packed, self.status, C.byref(n)))
        return n.value


def range_decomposition(upper_bound: int) -> str:
    """``RangeDecomposition::optimal(upper_bound).to_string()`` by the product's host code (no GPU needed)."""
    b = C.create_string_buffer(1024)
    _check(_load().eg_range_decomposition(upper_bound, b, 1024))
    return b.value.decode()


def plan_describe(kind: str, n_options: int = 0, credits_or_bound: int = 0) -> dict:
    """Summary of the flattened verification plan (host logic only, no GPU needed)."""
    import json

    kinds = {"single": 0, "multi": 1, "qv": 2, "zero": 3, "bool": 4, "range": 5, "sumsq": 6, "commit_equiv": 7}
    b = C.create_string_buffer(4096)
    _check(_load().eg_plan_describe(kinds[kind], n_options, credits_or_bound, b, 4096))
    return json.loads(b.value.decode())


def exported_symbols():
    """Names declared in include/eg_hip.h that the library must export (used by the CPU-side ABI test)."""
    import re

    hdr = (_PKG.parent / "include" / "eg_hip.h").read_text()
    return sorted(set(re.findall(r"\b(eg_[a-z0-9_]+)\s*\(", hdr)))


def _check(rc: int) -> None:
    if rc != 0:
        raise EgError(f"libeg_hip error {rc}: {_load().eg_last_error().decode()}")


class Context:
    """One GPU context per process (eg_init).  No reference analogue: the backend there is a ZST."""

    def __init__(self, device: int = 0):
        lib = _load()
        self._h = C.c_void_p()
        _check(lib.eg_init(device, C.byref(self._h)))
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            _load().eg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def name(self) -> str:
        b = C.create_string_buffer(256)
        _check(_load().eg_device_name(self._h, b, 256))
        return b.value.decode()

    def synchronize(self):
        _check(_load().eg_synchronize(self._h))

    def points_sum_device(self, n_ranks: int, n_points: int, d_in: int, d_out: int, stream: int = 0, d_bad: int = 0):
        """d_out[k] = sum over ranks of d_in[r][k] (32-byte encodings): merge of all-gathered per-GPU tallies.
        d_bad: device uint32 counter (zeroed by the caller) of slots that received an undecodable encoding."""
        _check(_load().eg_points_sum_device(self._h, n_ranks, n_points, d_in, d_out, d_bad or None, stream))

    @staticmethod
    def weed_index_bytes(board_cap: int) -> int:
        """Bytes of a board index (include/eg_hip.h, "persistent board index") over a board with room for board_cap ciphertexts; 0 for
        board_cap >= 2^31."""
        return int(_load().eg_weed_index_bytes(board_cap))

    def weed_index_build_device(self, n_prior: int, d_board: int, board_cap: int, index_seed: int, d_index: int, d_found: int, stream: int = 0):
        """eg_weed_index_build_device: clears the index and inserts board entries [0, n_prior); asynchronous on `stream`.  d_found: one
        uint32 the library writes, non-zero if the index overflowed."""
        _check(_load().eg_weed_index_build_device(self._h, n_prior, d_board or None, board_cap, index_seed & 0xFFFFFFFFFFFFFFFF, d_index or None,
                                                  d_found or None, stream or None))

    def weed_index_find_device(self, n_q: int, d_keys: int, n_prior: int, d_board: int, board_cap: int, d_index: int, index_seed: int, d_pos: int,
                               stream: int = 0):
        """eg_weed_index_find_device: d_pos[q] (uint32) = the smallest board position that holds the 64 bytes of key q, or DUP_NONE.  The
        index is only read."""
        _check(_load().eg_weed_index_find_device(self._h, n_q, d_keys or None, n_prior, d_board or None, board_cap, d_index or None,
                                                 index_seed & 0xFFFFFFFFFFFFFFFF, d_pos or None, stream or None))

    def merlin_challenges(self, proto: bytes, msg_label: bytes, msgs, chal_label: bytes, out_len: int = 64):
        """``Transcript::new(proto); append_message(msg_label, m); challenge_bytes(chal_label, out_len)`` for every message m
        (all of one length) on the GPU: the transcript layer of proofs/mod.rs:39-57 as a primitive."""
        msgs = list(msgs)
        n = len(msgs)
        ml = len(msgs[0]) if n else 0
        if any(len(m) != ml for m in msgs):
            raise ValueError("messages must have one length")
        out = C.create_string_buffer(max(n * out_len, 1))
        _check(_load().eg_merlin_challenge_batch(self._h, n, proto, len(proto), msg_label, len(msg_label), b"".join(msgs), ml,
                                                 chal_label, len(chal_label), out, out_len))
        return [out.raw[i * out_len : (i + 1) * out_len] for i in range(n)]

    def profile_enable(self, on=True):
        """on = 2: profile and run the chunks of a call serially on one work set (a launch's duration is then its own)."""
        _check(_load().eg_profile_enable(self._h, int(on)))

    def profile_read(self):
        """(dominant-kernel ms total, launches, whole-verify ms total) since the last read; HIP events."""
        a, n, b = C.c_double(), C.c_uint64(), C.c_double()
        _check(_load().eg_profile_read(self._h, C.byref(a), C.byref(n), C.byref(b)))
        return a.value, n.value, b.value

    def profile_read_tables(self):
        """(k_base_tables ms total, launches) for the launches folded in by the last profile_read()."""
        a, n = C.c_double(), C.c_uint64()
        _check(_load().eg_profile_read_tables(self._h, C.byref(a), C.byref(n)))
        return a.value, n.value


    def selfbench_fmul(self, seconds: float = 2.0):
        """(G field multiplications/s, shader clock MHz) of the shipped fe_mul in a bare chain sustained for `seconds` on this box
        (eg_selfbench_fmul): the VALU roof bench.py quotes its fractions against."""
        g, f = C.c_double(), C.c_double()
        _check(_load().eg_selfbench_fmul(self._h, float(seconds), C.byref(g), C.byref(f)))
        return g.value, f.value

    def comb_table_bits(self):
        """(window bits of the comb tables built at start-up, window bits of the wide tables or 0 while they do not exist)."""
        a, b = C.c_int(), C.c_int()
        _check(_load().eg_comb_table_bits(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def selfcheck_generator_table(self, wide: bool = False, samples: int = 4096, seed: int = 1) -> int:
        """Entries of the generator's comb table that differ from an entry-by-entry recomputation (must be 0); wide=True
        checks (and first builds) the wide table that large batches use."""
        bad = C.c_uint64()
        _check(_load().eg_selfcheck_generator_table(self._h, int(wide), samples, seed, C.byref(bad)))
        return bad.value


class Ristretto:
    """Batched ``Group`` backend for Ristretto255 (src/group/ristretto.rs).  All arguments are concatenated
    32-byte encodings (64-byte for wide scalars); every method runs one GPU lane per problem."""

    SCALAR_SIZE = 32
    ELEMENT_SIZE = 32

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def scalar_from_random_bytes(self, wide: bytes) -> bytes:  # ristretto.rs:34-38
        n = len(wide) // 64
        out = C.create_string_buffer(32 * n)
        _check(_load().eg_scalar_from_wide_batch(self.ctx._h, n, wide, out))
        return out.raw

    def deserialize_scalar_ok(self, scalars: bytes) -> bytes:  # ristretto.rs:59-62
        n = len(scalars) // 32
        ok = C.create_string_buffer(n)
        _check(_load().eg_scalar_is_canonical_batch(self.ctx._h, n, scalars, ok))
        return ok.raw

    def scalar_muladd(self, a: bytes, b: bytes, c: bytes) -> bytes:
        n = len(a) // 32
        out = C.create_string_buffer(32 * n)
        _check(_load().eg_scalar_muladd_batch(self.ctx._h, n, a, b, c, out))
        return out.raw

    def scalar_neg(self, a: bytes) -> bytes:
        n = len(a) // 32
        out = C.create_string_buffer(32 * n)
        _check(_load().eg_scalar_neg_batch(self.ctx._h, n, a, out))
        return out.raw

    def invert_scalars(self, a: bytes) -> bytes:  # group/mod.rs:104-118, ristretto.rs:40-52
        n = len(a) // 32
        out = C.create_string_buffer(32 * n)
        _check(_load().eg_scalar_invert_batch(self.ctx._h, n, a, out))
        return out.raw

    def is_identity(self, elements: bytes):
        """ElementOps::is_identity (ristretto.rs:80-82): (is_identity flags, ok flags)."""
        n = len(elements) // 32
        f, ok = C.create_string_buffer(n), C.create_string_buffer(n)
        _check(_load().eg_point_is_identity_batch(self.ctx._h, n, elements, f, ok))
        return f.raw, ok.raw

    def element_neg(self, a: bytes):
        return self.element_add(bytes(len(a)), a, subtract=True)

    def element_roundtrip(self, elements: bytes):
        """deserialize_element + serialize_element (ristretto.rs:88-95): (re-encodings, ok flags)."""
        n = len(elements) // 32
        out, ok = C.create_string_buffer(32 * n), C.create_string_buffer(n)
        _check(_load().eg_point_roundtrip_batch(self.ctx._h, n, elements, out, ok))
        return out.raw, ok.raw

    def element_add(self, a: bytes, b: bytes, subtract: bool = False):
        n = len(a) // 32
        out, ok = C.create_string_buffer(32 * n), C.create_string_buffer(n)
        _check(_load().eg_point_add_batch(self.ctx._h, n, a, b, int(subtract), out, ok))
        return out.raw, ok.raw

    def mul_generator(self, k: bytes) -> bytes:  # ristretto.rs:105-121
        n = len(k) // 32
        out = C.create_string_buffer(32 * n)
        _check(_load().eg_mul_generator_batch(self.ctx._h, n, k, out))
        return out.raw

    def vartime_double_mul_generator(self, k: bytes, p: bytes, r: bytes):  # ristretto.rs:131-137
        n = len(k) // 32
        out, ok = C.create_string_buffer(32 * n), C.create_string_buffer(n)
        _check(_load().eg_vartime_double_mul_generator_batch(self.ctx._h, n, k, p, r, out, ok))
        return out.raw, ok.raw

    def vartime_multi_mul(self, terms: int, scalars: bytes, points: bytes):  # ristretto.rs:139-145
        n = len(scalars) // (32 * terms) if terms else 0
        out, ok = C.create_string_buffer(32 * max(n, 1)), C.create_string_buffer(max(n, 1))
        _check(_load().eg_vartime_multi_mul_batch(self.ctx._h, n, terms, scalars, points, out, ok))
        return out.raw[: 32 * n], ok.raw[:n]

    def msm_scratch_bytes(self, n: int, terms: int) -> int:
        return int(_load().eg_msm_scratch_bytes_ctx(self.ctx._h, n, terms))

    def prepare_points_device(self, n: int, d_encodings: int, d_prepared: int, d_ok: int, stream: int = 0):
        """Decodes n elements once into prepared points (prepared_point_size() bytes each, 16-byte aligned) for repeated products over
        them.  d_ok (n bytes, device) is mandatory: an encoding that does not decode is prepared as the identity, and this is the only
        place that says so."""
        _check(_load().eg_points_prepare_device(self.ctx._h, n, d_encodings, d_prepared, d_ok, stream))

    def vartime_multi_mul_prepared_device(self, n: int, terms: int, d_scalars: int, d_prepared: int, d_out: int, d_r: int = 0, d_scratch: int = 0,
                                          stream: int = 0):
        """vartime_multi_mul over prepared points (no decoding per term)."""
        _check(_load().eg_vartime_multi_mul_prepared_batch_device(self.ctx._h, n, terms, d_scalars, d_prepared, d_r, d_scratch, d_out, stream))

    def vartime_multi_mul_device(self, n: int, terms: int, d_scalars: int, d_points: int, d_out: int, d_r: int = 0, d_scratch: int = 0,
                                 d_ok: int = 0, stream: int = 0):
        """The multi-scalar multiplication on device buffers, asynchronous on `stream` (eg_vartime_multi_mul_batch_device)."""
        _check(_load().eg_vartime_multi_mul_batch_device(self.ctx._h, n, terms, d_scalars, d_points, d_r, d_scratch, d_out, d_ok, stream))


class Ed25519:
    """Voter signatures: Ed25519 (RFC 8032, pure EdDSA) of a batch in one pass (include/eg_hip.h, "voter signatures" has the rule).
    Item b signs prefix || msgs[b * stride : b * stride + msg_len] under keys[b], or under keys[key_index[b]] out of a roster.
    The signer (keypairs, sign) is VARIABLE TIME: a maker of test and benchmark items, not for a voter client."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    @staticmethod
    def _n(msgs: bytes, msg_len: int, stride, n):
        stride = msg_len if stride is None else stride
        if n is None:
            if stride == 0:
                raise EgError("n is needed for messages of length 0")
            n = (len(msgs) + stride - msg_len) // stride
        return n, stride

    def keypairs(self, seeds: bytes) -> bytes:
        """Public keys (32 bytes each) of the 32-byte seeds."""
        n = len(seeds) // 32
        out = C.create_string_buffer(32 * n)
        _check(_load().eg_ed25519_keypair_batch(self.ctx._h, n, seeds, out))
        return out.raw

    def sign(self, seeds: bytes, msgs: bytes, msg_len: int, prefix: bytes = b"", stride=None) -> bytes:
        """Signatures (64 bytes each): item b is signed under seeds[b]."""
        n = len(seeds) // 32
        _, stride = self._n(msgs, msg_len, stride, n)
        out = C.create_string_buffer(64 * n)
        _check(_load().eg_ed25519_sign_batch(self.ctx._h, n, seeds, msgs, stride, msg_len, prefix or None, len(prefix), out))
        return out.raw

    def verify(self, msgs: bytes, msg_len: int, keys: bytes, sigs: bytes, prefix: bytes = b"", key_index=None, status_in=None, stride=None):
        """Status words of the n = len(sigs) / 64 items: 0, or ST_BAD_SIGNATURE with the failed check in status_detail; a non-zero word
        of status_in is handed on and that item is not looked at."""
        import array

        n = len(sigs) // 64
        _, stride = self._n(msgs, msg_len, stride, n)
        idx = (C.c_uint32 * n)(*key_index) if key_index is not None else None
        sin = (C.c_uint32 * n)(*status_in) if status_in is not None else None
        out = (C.c_uint32 * max(n, 1))()
        _check(_load().eg_ed25519_verify_batch(self.ctx._h, n, msgs, stride, msg_len, prefix or None, len(prefix), keys, len(keys) // 32, idx, sigs,
                                               sin, out))
        return array.array("I", out[:n]).tolist()

    def verify_scratch_bytes(self, n: int) -> int:
        return int(_load().eg_ed25519_verify_scratch_bytes(self.ctx._h, n))

    def verify_device(self, n: int, d_msgs: int, msg_stride: int, msg_len: int, d_keys: int, n_keys: int, d_sigs: int, d_status_out: int,
                      d_scratch: int, scratch_bytes: int, prefix: bytes = b"", d_key_index: int = 0, d_status_in: int = 0, stream: int = 0):
        """Asynchronous device-pointer variant (eg_ed25519_verify_device): no allocation, no host synchronisation, no lock.  `prefix` is
        host bytes; d_scratch: verify_scratch_bytes(n) bytes; d_status_out may be d_status_in."""
        _check(_load().eg_ed25519_verify_device(self.ctx._h, n, d_msgs or None, msg_stride, msg_len, prefix or None, len(prefix), d_keys or None,
                                                n_keys, d_key_index or None, d_sigs or None, d_status_in or None, d_status_out or None,
                                                d_scratch or None, scratch_bytes, stream or None))

    def keypairs_device(self, n: int, d_seeds: int, d_keys: int, stream: int = 0):
        _check(_load().eg_ed25519_keypair_batch_device(self.ctx._h, n, d_seeds or None, d_keys or None, stream or None))

    def sign_device(self, n: int, d_seeds: int, d_msgs: int, msg_stride: int, msg_len: int, d_sigs: int, d_prefix: int = 0, prefix_len: int = 0,
                    stream: int = 0):
        _check(_load().eg_ed25519_sign_batch_device(self.ctx._h, n, d_seeds or None, d_msgs or None, msg_stride, msg_len, d_prefix or None,
                                                    prefix_len, d_sigs or None, stream or None))

    def sha512(self, msgs: bytes, msg_len: int, prefix: bytes = b"", stride=None, n=None) -> bytes:
        """SHA-512(prefix || msg_b) of n messages of one length: 64 bytes each."""
        n, stride = self._n(msgs, msg_len, stride, n)
        out = C.create_string_buffer(64 * max(n, 1))
        _check(_load().eg_sha512_batch(self.ctx._h, n, msgs, stride, msg_len, prefix or None, len(prefix), out))
        return out.raw[: 64 * n]

    def sha512_device(self, n: int, d_msgs: int, msg_stride: int, msg_len: int, d_digests: int, d_prefix: int = 0, prefix_len: int = 0, stream: int = 0):
        _check(_load().eg_sha512_batch_device(self.ctx._h, n, d_msgs or None, msg_stride, msg_len, d_prefix or None, prefix_len, d_digests or None,
                                              stream or None))


class RollResult:
    """What VoterRoll.cast / check say about a batch: per ballot superseded_by (SEQ_NONE: kept, not participating, or without a winner),
    status_out, groups_out / weights_out (None without a roster array); displaced = [(old seq, new seq), ...] (cast only); found = the
    three counters (superseded, displaced - check: not cast -, off the roll)."""

    def __init__(self, superseded_by, status_out, groups_out, weights_out, displaced, found):
        self.superseded_by, self.status_out, self.groups_out, self.weights_out = superseded_by, status_out, groups_out, weights_out
        self.displaced, self.found = displaced, found

    def kept(self, status_in=None):
        """Indices of the ballots that count: they participate and their status word came through unchanged."""
        return [b for b, s in enumerate(self.status_out) if s == 0 and (status_in is None or status_in[b] == 0)]


class VoterRoll:
    """One counted ballot per voter (include/eg_hip.h, "voter roll" has the rule): between weeding and the tally.  The roll is the caller's
    list of n_keys 64-bit words (0 = no counted ballot yet), kept between calls; `policy` is ROLL_LAST or ROLL_FIRST and a roll belongs to
    one policy.  Rolls of slabs, ranks or GPUs merge by the element-wise maximum (distributed.merge_rolls)."""

    ST_SUPERSEDED, ROLL_FIRST, ROLL_LAST = ST_SUPERSEDED, ROLL_FIRST, ROLL_LAST
    ROLL_SUPERSEDED, ROLL_OFF_ROLL, ROLL_NOT_CAST = ROLL_SUPERSEDED, ROLL_OFF_ROLL, ROLL_NOT_CAST
    SEQ_NONE, ROLL_KEYS_MAX = SEQ_NONE, ROLL_KEYS_MAX

    def __init__(self, ctx: Context, policy: int = ROLL_LAST):
        self.ctx, self.policy = ctx, policy

    def word(self, seq: int) -> int:
        """EG_ROLL_WORD: the priority word of sequence number seq under this roll's policy."""
        return seq + 1 if self.policy == ROLL_LAST else (1 << 63) - 1 - seq

    def seq(self, word: int) -> int:
        """EG_ROLL_SEQ: the sequence number behind a non-zero word."""
        return word - 1 if self.policy == ROLL_LAST else (1 << 63) - 1 - word

    def _host(self, cast: bool, key_index, roll, seq_base, status_in, roster_groups, roster_weights, want_displaced):
        n, n_keys = len(key_index), len(roll)
        idx = (C.c_uint32 * max(n, 1))(*key_index)
        sin = (C.c_uint32 * max(n, 1))(*status_in) if status_in is not None else None
        words = (C.c_uint64 * max(n_keys, 1))(*roll)
        rg = (C.c_uint32 * max(n_keys, 1))(*roster_groups) if roster_groups is not None else None
        rw = (C.c_uint64 * max(n_keys, 1))(*roster_weights) if roster_weights is not None else None
        by, out = (C.c_uint64 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
        go = (C.c_uint32 * max(n, 1))() if rg is not None else None
        wo = (C.c_uint64 * max(n, 1))() if rw is not None else None
        found = (C.c_uint32 * 3)()
        lib = _load()
        if cast:
            disp = (C.c_uint64 * max(2 * n, 1))() if want_displaced else None
            count = C.c_uint64(0)
            _check(lib.eg_roll_cast(self.ctx._h, n, idx, sin, seq_base, self.policy, words, n_keys, rg, rw, by, out, go, wo, disp,
                                    C.byref(count) if want_displaced else None, found))
            displaced = [(int(disp[2 * k]), int(disp[2 * k + 1])) for k in range(count.value)] if want_displaced else None
        else:
            _check(lib.eg_roll_check(self.ctx._h, n, idx, sin, seq_base, self.policy, words, n_keys, rg, rw, by, out, go, wo, found))
            displaced = None
        res = RollResult(list(by[:n]), list(out[:n]), list(go[:n]) if go is not None else None, list(wo[:n]) if wo is not None else None,
                         displaced, list(found))
        return res, list(words[:n_keys])

    def cast(self, key_index, roll, seq_base: int = 0, status_in=None, roster_groups=None, roster_weights=None, displaced: bool = True):
        """eg_roll_cast: (RollResult, the new roll).  key_index[b] = the roster index of the voter who signed ballot b, whose sequence
        number is seq_base + b; a ballot participates iff its word of status_in is 0 (None: every ballot)."""
        return self._host(True, key_index, roll, seq_base, status_in, roster_groups, roster_weights, displaced)

    def check(self, key_index, roll, seq_base: int = 0, status_in=None, roster_groups=None, roster_weights=None) -> RollResult:
        """eg_roll_check: the verdicts of a batch against a read-only roll (the final one, or a merged one)."""
        return self._host(False, key_index, roll, seq_base, status_in, roster_groups, roster_weights, False)[0]

    def cast_scratch_bytes(self, n: int, n_keys: int) -> int:
        """Device scratch that cast_device needs (0 for arguments it refuses, and for n == 0)."""
        return int(_load().eg_roll_cast_scratch_bytes(self.ctx._h, n, n_keys))

    def cast_device(self, n: int, d_key_index: int, seq_base: int, d_roll: int, n_keys: int, d_superseded_by: int, d_found: int, d_scratch: int,
                    scratch_bytes: int, d_status_in: int = 0, d_roster_groups: int = 0, d_roster_weights: int = 0, d_status_out: int = 0,
                    d_groups_out: int = 0, d_weights_out: int = 0, d_displaced: int = 0, d_displaced_count: int = 0, stream: int = 0):
        """Asynchronous device-pointer variant (eg_roll_cast_device): no allocation, no host synchronisation, no lock.  d_roll: n_keys uint64,
        read and written; d_superseded_by: n uint64; d_found: 3 uint32; d_displaced: n x 2 uint64 with d_displaced_count (uint64), or both 0;
        d_status_out may be d_status_in."""
        _check(_load().eg_roll_cast_device(self.ctx._h, n, d_key_index or None, d_status_in or None, seq_base, self.policy, d_roll or None, n_keys,
                                           d_roster_groups or None, d_roster_weights or None, d_superseded_by or None, d_status_out or None,
                                           d_groups_out or None, d_weights_out or None, d_displaced or None, d_displaced_count or None,
                                           d_found or None, d_scratch or None, scratch_bytes, stream or None))

    def check_device(self, n: int, d_key_index: int, seq_base: int, d_roll: int, n_keys: int, d_superseded_by: int, d_found: int,
                     d_status_in: int = 0, d_roster_groups: int = 0, d_roster_weights: int = 0, d_status_out: int = 0, d_groups_out: int = 0,
                     d_weights_out: int = 0, stream: int = 0):
        """Asynchronous device-pointer variant (eg_roll_check_device): the roll is only read."""
        _check(_load().eg_roll_check_device(self.ctx._h, n, d_key_index or None, d_status_in or None, seq_base, self.policy, d_roll or None, n_keys,
                                            d_roster_groups or None, d_roster_weights or None, d_superseded_by or None, d_status_out or None,
                                            d_groups_out or None, d_weights_out or None, d_found or None, stream or None))


class LeafResult:
    """What ReceiptLog.leaves says about a batch: leaf_index per ballot (LEAF_NONE: it does not participate), leaves = the n x 32 bytes of
    leaves_out (zeroed rows for ballots that do not participate), log = the caller's log with the participating leaves appended (None
    without an append), found = (number of leaves, non-zero: the append did not fit)."""

    def __init__(self, leaf_index, leaves, log, found):
        self.leaf_index, self.leaves, self.log, self.found = leaf_index, leaves, log, found


class ReceiptLog:
    """Ballot receipts (include/eg_hip.h, "receipt log" has the rule): a Merkle tree (RFC 6962, H = the first 32 bytes of SHA-512) over
    the posted ballots.  The log is the caller's bytes of 32-byte leaves, normally fed weeding's status_out; `prefix` is the election id.
    Every tree() is a full rebuild; there is no incremental frontier state.  grow() builds the store of the grown log out of the store of
    the last head and hashes only what the append changed."""

    BAD_INDEX, BAD_LENGTH, MISMATCH = MERKLE_BAD_INDEX, MERKLE_BAD_LENGTH, MERKLE_MISMATCH
    MISMATCH_OLD = MERKLE_MISMATCH_OLD
    HASH_BYTES, LEAVES_MAX, LEAF_NONE, NO_PATH = MERKLE_HASH_BYTES, MERKLE_LEAVES_MAX, LEAF_NONE, MERKLE_NO_PATH

    def __init__(self, ctx: Context, prefix: bytes = b""):
        self.ctx, self.prefix = ctx, bytes(prefix)

    @staticmethod
    def depth(n_leaves: int) -> int:
        """eg_merkle_depth: ceil(log2 N), 0 for N <= 1 (pure host arithmetic)."""
        return int(_load().eg_merkle_depth(n_leaves))

    @staticmethod
    def nodes_bytes(n_leaves: int) -> int:
        """eg_merkle_nodes_bytes: the size of the node store (levels 1 .. depth back to back)."""
        return int(_load().eg_merkle_nodes_bytes(n_leaves))

    @staticmethod
    def level(n_leaves: int, level: int):
        """eg_merkle_level: (byte offset into the node store, node count) of a level; level 0 is the log itself."""
        off, count = C.c_uint64(0), C.c_uint64(0)
        _check(_load().eg_merkle_level(n_leaves, level, C.byref(off), C.byref(count)))
        return int(off.value), int(count.value)

    def leaves(self, msgs: bytes, msg_len: int, extra: bytes = None, extra_len: int = 0, status_in=None, log: bytes = None, log_cap: int = None,
               n_prior: int = None, stride=None, extra_stride=None, n=None) -> LeafResult:
        """eg_merkle_leaves: the leaf of every participating ballot (status_in None: all).  With `log` (bytes of earlier leaves) the
        participating leaves are appended behind it, at most log_cap entries in all (None: whatever is needed); without one n_prior
        (default 0) still counts into leaf_index.  Raises EgError after the outputs are lost if the append does not fit."""
        n, stride = Ed25519._n(msgs, msg_len, stride, n)
        extra_stride = extra_len if extra_stride is None else extra_stride
        append = log is not None
        if append:
            n_prior = len(log) // MERKLE_HASH_BYTES
            log_cap = n_prior + n if log_cap is None else log_cap
        n_prior = n_prior or 0
        sin = (C.c_uint32 * max(n, 1))(*status_in) if status_in is not None else None
        idx = (C.c_uint64 * max(n, 1))()
        out = C.create_string_buffer(MERKLE_HASH_BYTES * max(n, 1))
        room = None
        if append:
            room = C.create_string_buffer(MERKLE_HASH_BYTES * max(log_cap, n_prior, 1))
            C.memmove(room, bytes(log), MERKLE_HASH_BYTES * n_prior)
        count, found = C.c_uint64(0), (C.c_uint32 * 2)()
        _check(_load().eg_merkle_leaves(self.ctx._h, n, msgs, stride, msg_len, self.prefix or None, len(self.prefix), extra if extra_len else None,
                                        extra_stride, extra_len, sin, n_prior, idx, out, room, log_cap or 0, C.byref(count) if append else None, found))
        return LeafResult(list(idx[:n]), out.raw[: MERKLE_HASH_BYTES * n], room.raw[: MERKLE_HASH_BYTES * count.value] if append else None, list(found))

    def tree(self, log: bytes, with_nodes: bool = True):
        """eg_merkle_tree: (root, node store or None) over the len(log) / 32 leaves of the log; a full rebuild."""
        n = len(log) // MERKLE_HASH_BYTES
        root = C.create_string_buffer(MERKLE_HASH_BYTES)
        size = self.nodes_bytes(n)
        nodes = C.create_string_buffer(max(size, 1)) if with_nodes else None
        _check(_load().eg_merkle_tree(self.ctx._h, n, log or None, root, nodes))
        return root.raw, (nodes.raw[:size] if with_nodes else None)

    def paths(self, index, log: bytes, nodes: bytes):
        """eg_merkle_paths: ([path bytes per requested leaf, or None for an index that is not in the log], the raw rows, path_len)."""
        n, m = len(log) // MERKLE_HASH_BYTES, len(index)
        row = MERKLE_HASH_BYTES * self.depth(n)
        idx = (C.c_uint64 * max(m, 1))(*index)
        out = C.create_string_buffer(max(m * row, 1))
        lens = (C.c_uint32 * max(m, 1))()
        _check(_load().eg_merkle_paths(self.ctx._h, m, idx, n, log or None, nodes or None, out if row else None, lens))
        rows = out.raw[: m * row]
        paths = [None if lens[j] == MERKLE_NO_PATH else rows[j * row: j * row + MERKLE_HASH_BYTES * lens[j]] for j in range(m)]
        return paths, rows, list(lens[:m])

    def check(self, index, leaves: bytes, paths, n_leaves: int, root: bytes, path_len=None, path_stride=None):
        """eg_merkle_check: (verdicts, found).  `paths` is a list of path bytes (their lengths are the path_len), or raw rows with path_len
        and path_stride given."""
        m = len(index)
        if path_len is None:
            path_len = [len(p) // MERKLE_HASH_BYTES for p in paths]
            path_stride = max([MERKLE_HASH_BYTES * self.depth(n_leaves)] + [len(p) for p in paths])
            paths = b"".join(p + bytes(path_stride - len(p)) for p in paths)
        idx = (C.c_uint64 * max(m, 1))(*index)
        lens = (C.c_uint32 * max(m, 1))(*path_len)
        verdict, found = (C.c_uint32 * max(m, 1))(), (C.c_uint32 * 3)()
        _check(_load().eg_merkle_check(self.ctx._h, m, idx, leaves, paths or None, path_stride, lens, n_leaves, root, verdict, found))
        return list(verdict[:m]), list(found)

    @staticmethod
    def leaves_scratch_bytes(n: int) -> int:
        return int(_load().eg_merkle_leaves_scratch_bytes(n))

    @staticmethod
    def tree_scratch_bytes(n_leaves: int) -> int:
        """Scratch of tree_device WITHOUT a node store (0 up to 1024 leaves)."""
        return int(_load().eg_merkle_tree_scratch_bytes(n_leaves))

    def leaves_device(self, n: int, d_msgs: int, msg_stride: int, msg_len: int, d_leaf_index: int, d_found: int, d_scratch: int, scratch_bytes: int,
                      d_extra: int = 0, extra_stride: int = 0, extra_len: int = 0, d_status_in: int = 0, n_prior: int = 0, d_leaves_out: int = 0,
                      d_log: int = 0, log_cap: int = 0, d_log_count: int = 0, stream: int = 0):
        """Asynchronous device-pointer variant (eg_merkle_leaves_device): no allocation, no host synchronisation, no lock.  d_leaf_index: n
        uint64; d_found: 2 uint32; d_log (log_cap x 32) with d_log_count (uint64) requests the append."""
        _check(_load().eg_merkle_leaves_device(self.ctx._h, n, d_msgs or None, msg_stride, msg_len, self.prefix or None, len(self.prefix),
                                               d_extra or None, extra_stride, extra_len, d_status_in or None, n_prior, d_leaf_index or None,
                                               d_leaves_out or None, d_log or None, log_cap, d_log_count or None, d_found or None,
                                               d_scratch or None, scratch_bytes, stream or None))

    def tree_device(self, n_leaves: int, d_log: int, d_root: int, d_nodes: int = 0, d_scratch: int = 0, scratch_bytes: int = 0, stream: int = 0):
        _check(_load().eg_merkle_tree_device(self.ctx._h, n_leaves, d_log or None, d_root or None, d_nodes or None, d_scratch or None, scratch_bytes,
                                             stream or None))

    def paths_device(self, m: int, d_index: int, n_leaves: int, d_log: int, d_nodes: int, d_paths: int, d_path_len: int, stream: int = 0):
        _check(_load().eg_merkle_paths_device(self.ctx._h, m, d_index or None, n_leaves, d_log or None, d_nodes or None, d_paths or None,
                                              d_path_len or None, stream or None))

    def check_device(self, m: int, d_index: int, d_leaves: int, d_paths: int, path_stride: int, d_path_len: int, n_leaves: int, d_root: int,
                     d_verdict: int, d_found: int, stream: int = 0):
        _check(_load().eg_merkle_check_device(self.ctx._h, m, d_index or None, d_leaves or None, d_paths or None, path_stride, d_path_len or None,
                                              n_leaves, d_root or None, d_verdict or None, d_found or None, stream or None))

    # ---- past heads and consistency proofs: "the board that published (m, R_m) is the same board, grown, that now publishes (N, R_N)"
    @staticmethod
    def consistency_len(old_size: int, n_leaves: int) -> int:
        """eg_merkle_consistency_len: the length of the consistency proof of (old_size, N); NO_PATH for old_size 0 or above N."""
        return int(_load().eg_merkle_consistency_len(old_size, n_leaves))

    def heads(self, sizes, log: bytes, nodes: bytes):
        """eg_merkle_heads: ([the head the log had at each size], found).  Size 0 gives H(""), a size above N a zeroed head, counted in
        found[0]."""
        n, m = len(log) // MERKLE_HASH_BYTES, len(sizes)
        arr = (C.c_uint64 * max(m, 1))(*sizes)
        out = C.create_string_buffer(MERKLE_HASH_BYTES * max(m, 1))
        found = (C.c_uint32 * 1)()
        _check(_load().eg_merkle_heads(self.ctx._h, m, arr, n, log or None, nodes or None, out, found))
        return [out.raw[MERKLE_HASH_BYTES * j: MERKLE_HASH_BYTES * (j + 1)] for j in range(m)], list(found)

    def consistency(self, old_sizes, log: bytes, nodes: bytes):
        """eg_merkle_consistency: ([proof bytes per old size, or None for an old size that is 0 or above N], the raw rows of depth(N) + 1
        entries, proof_len)."""
        n, m = len(log) // MERKLE_HASH_BYTES, len(old_sizes)
        row = MERKLE_HASH_BYTES * (self.depth(n) + 1)
        arr = (C.c_uint64 * max(m, 1))(*old_sizes)
        out = C.create_string_buffer(max(m * row, 1))
        lens = (C.c_uint32 * max(m, 1))()
        _check(_load().eg_merkle_consistency(self.ctx._h, m, arr, n, log or None, nodes or None, out, lens))
        rows = out.raw[: m * row]
        proofs = [None if lens[j] == MERKLE_NO_PATH else rows[j * row: j * row + MERKLE_HASH_BYTES * lens[j]] for j in range(m)]
        return proofs, rows, list(lens[:m])

    def consistency_check(self, old_sizes, old_roots, proofs, n_leaves: int, root: bytes, proof_len=None, proof_stride=None):
        """eg_merkle_consistency_check: (verdicts, found[4]).  `old_roots` is a list of heads or their bytes back to back; `proofs` is a
        list of proof bytes (their lengths are the proof_len), or raw rows with proof_len and proof_stride given."""
        m = len(old_sizes)
        if not isinstance(old_roots, (bytes, bytearray)):
            old_roots = b"".join(old_roots)
        if proof_len is None:
            proof_len = [len(p) // MERKLE_HASH_BYTES for p in proofs]
            proof_stride = max([MERKLE_HASH_BYTES * (self.depth(n_leaves) + 1)] + [len(p) for p in proofs])
            proofs = b"".join(p + bytes(proof_stride - len(p)) for p in proofs)
        arr = (C.c_uint64 * max(m, 1))(*old_sizes)
        lens = (C.c_uint32 * max(m, 1))(*proof_len)
        verdict, found = (C.c_uint32 * max(m, 1))(), (C.c_uint32 * 4)()
        _check(_load().eg_merkle_consistency_check(self.ctx._h, m, arr, bytes(old_roots) or None, proofs or None, proof_stride, lens, n_leaves, root,
                                                   verdict, found))
        return list(verdict[:m]), list(found)

    def heads_device(self, m: int, d_size: int, n_leaves: int, d_log: int, d_nodes: int, d_heads: int, d_found: int, stream: int = 0):
        """Asynchronous device-pointer variant (eg_merkle_heads_device).  d_size: m uint64; d_heads: m x 32; d_found: 1 uint32."""
        _check(_load().eg_merkle_heads_device(self.ctx._h, m, d_size or None, n_leaves, d_log or None, d_nodes or None, d_heads or None,
                                              d_found or None, stream or None))

    def consistency_device(self, m: int, d_old_size: int, n_leaves: int, d_log: int, d_nodes: int, d_proofs: int, d_proof_len: int, stream: int = 0):
        """eg_merkle_consistency_device.  d_proofs: m rows of depth(N) + 1 entries; d_proof_len: m uint32."""
        _check(_load().eg_merkle_consistency_device(self.ctx._h, m, d_old_size or None, n_leaves, d_log or None, d_nodes or None, d_proofs or None,
                                                    d_proof_len or None, stream or None))

    def consistency_check_device(self, m: int, d_old_size: int, d_old_root: int, d_proofs: int, proof_stride: int, d_proof_len: int, n_leaves: int,
                                 d_root: int, d_verdict: int, d_found: int, stream: int = 0):
        """eg_merkle_consistency_check_device.  d_found: 4 uint32 (BAD_INDEX, BAD_LENGTH, MISMATCH, MISMATCH_OLD)."""
        _check(_load().eg_merkle_consistency_check_device(self.ctx._h, m, d_old_size or None, d_old_root or None, d_proofs or None, proof_stride,
                                                          d_proof_len or None, n_leaves, d_root or None, d_verdict or None, d_found or None,
                                                          stream or None))

    # ---- grow: the tree of N leaves out of the tree of its first m, hashing only what the append changed
    def grow(self, old_size: int, nodes_old: bytes, log: bytes):
        """eg_merkle_grow: (root, node store) over the len(log) / 32 leaves of the log, byte for byte what tree(log) returns, out of the
        node store of its first old_size leaves.  Only the tiles that hold a changed node are hashed again; nodes_old is left as it is."""
        n = len(log) // MERKLE_HASH_BYTES
        root = C.create_string_buffer(MERKLE_HASH_BYTES)
        size = self.nodes_bytes(n)
        nodes = C.create_string_buffer(max(size, 1))
        _check(_load().eg_merkle_grow(self.ctx._h, old_size, nodes_old or None, n, log or None, nodes, root))
        return root.raw, nodes.raw[:size]

    def grow_device(self, old_size: int, d_nodes_old: int, n_leaves: int, d_log: int, d_nodes: int, d_root: int, stream: int = 0):
        """Asynchronous device-pointer variant (eg_merkle_grow_device): no allocation, no scratch, no host synchronisation, no lock.  The
        two stores must not overlap."""
        _check(_load().eg_merkle_grow_device(self.ctx._h, old_size, d_nodes_old or None, n_leaves, d_log or None, d_nodes or None, d_root or None,
                                             stream or None))


class ShuffleVerifier:
    """Checks a mixer's proof of a re-encryption shuffle (include/eg_hip.h, "re-encryption shuffles" has the rule).  The commitment key
    H_0 .. H_cap is derived from `seed` once and serves every shuffle of at most `cap` rows; `K` is the election key.  verify() takes
    rows of 64 bytes (R || B) as bytes and returns (verdict mask, rows, found); 0 means accepted."""

    BAD_ENCODING, T1, T2, T3, T41, T42, CHAIN = 1, 2, 4, 8, 16, 32, 64
    ROW_BAD, ROW_CHAIN = SHUFFLE_ROW_BAD, SHUFFLE_ROW_CHAIN
    ROWS_MAX, KEY_TRIES = SHUFFLE_ROWS_MAX, SHUFFLE_KEY_TRIES

    def __init__(self, ctx: Context, K: bytes, seed: bytes = b"", cap: int = 0, key: bytes = None):
        self.ctx, self.K = ctx, bytes(K)
        self.key = bytes(key) if key is not None else self.derive_key(ctx, seed, cap)
        self.cap = len(self.key) // 32 - 1

    @staticmethod
    def key_bytes(cap: int) -> int:
        return int(_load().eg_shuffle_key_bytes(cap))

    @staticmethod
    def proof_bytes(n: int) -> int:
        return int(_load().eg_shuffle_proof_bytes(n))

    @staticmethod
    def derive_key(ctx: Context, seed: bytes, cap: int) -> bytes:
        """eg_shuffle_key_derive: the 32 (cap + 1) bytes of H_0 .. H_cap."""
        out = C.create_string_buffer(max(32 * (cap + 1), 1))
        _check(_load().eg_shuffle_key_derive(ctx._h, bytes(seed) or None, len(seed), cap, out))
        return out.raw[: 32 * (cap + 1)]

    def verify_scratch_bytes(self, n: int) -> int:
        return int(_load().eg_shuffle_verify_scratch_bytes(self.ctx._h, n))

    def verify(self, ins: bytes, outs: bytes, proof: bytes, prefix: bytes = b"", want_rows: bool = True):
        """eg_shuffle_verify: (verdict, rows or None, found)."""
        n = len(ins) // 64
        if len(outs) != 64 * n or len(proof) != 288 + 160 * n:
            raise EgError(f"a shuffle of {n} rows has {64 * n} output bytes and a proof of {288 + 160 * n} bytes")
        verdict, found = C.c_uint32(0), (C.c_uint32 * 4)()
        rows = (C.c_uint32 * max(n, 1))() if want_rows else None
        _check(_load().eg_shuffle_verify(self.ctx._h, n, ins or None, outs or None, self.K, bytes(prefix) or None, len(prefix), self.key, self.cap,
                                         proof or None, C.byref(verdict), rows, found))
        return int(verdict.value), (list(rows[:n]) if want_rows else None), list(found)

    def verify_device(self, n: int, d_in: int, d_out: int, d_key: int, d_proof: int, d_verdict: int, d_found: int, d_scratch: int, scratch_bytes: int,
                      prefix: bytes = b"", d_rows: int = 0, key_cap: int = None, stream: int = 0):
        """Asynchronous device-pointer variant (eg_shuffle_verify_device): no allocation, no host synchronisation.  d_key: a device copy of
        the key (32 (key_cap + 1) bytes); d_verdict: one uint32; d_found: 4 uint32; d_rows: n uint32 or 0."""
        _check(_load().eg_shuffle_verify_device(self.ctx._h, n, d_in or None, d_out or None, self.K, bytes(prefix) or None, len(prefix), d_key or None,
                                                self.cap if key_cap is None else key_cap, d_proof or None, d_verdict or None, d_rows or None,
                                                d_found or None, d_scratch or None, scratch_bytes, stream or None))

    def derive_key_device(self, seed: bytes, cap: int, d_key: int, d_exhausted: int, stream: int = 0):
        _check(_load().eg_shuffle_key_derive_device(self.ctx._h, bytes(seed) or None, len(seed), cap, d_key or None, d_exhausted or None, stream or None))


def prepared_point_size() -> int:
    return int(_load().eg_prepared_point_size())


def verify_batch_multi(per_device, ballots: bytes, with_tally: bool = True):
    """``eg_verify_*_batch_multi``: one batch over several params objects of the same election, each on its own context (normally one
    per GPU of the process): contiguous slabs, one host thread per object inside the library, tallies merged in the library.
    Returns (status words in ballot order, tally of this batch or None)."""
    per_device = list(per_device)
    p0 = per_device[0]
    if any(type(p) is not type(p0) for p in per_device):
        raise ValueError("params objects of different kinds")
    n = len(ballots) // p0.ballot_size
    if n * p0.ballot_size != len(ballots):
        raise ValueError("ballots is not a whole number of packed ballots")
    arr = (C.c_void_p * len(per_device))(*[p._h for p in per_device])
    st = (C.c_uint32 * max(n, 1))()
    tally = C.create_string_buffer(64 * p0.n_options) if with_tally else None
    buf = (C.c_char * max(len(ballots), 1)).from_buffer_copy(ballots or b"\0")
    fn = getattr(_load(), f"eg_verify_{p0._prefix}_batch_multi")
    _check(fn(arr, len(per_device), n, buf, st, tally))
    return list(st[:n]), (tally.raw if with_tally else None)


def verify_batch_multi_host_ptr(per_device, n: int, ballots_ptr: int, status_ptr: int, with_tally: bool = False):
    """``eg_verify_*_batch_multi`` on raw host addresses (e.g. ONE pinned torch tensor holding the whole batch): what a single-process
    host with its ballots in host memory calls; no Python-side copies.  Returns the tally of this batch or None."""
    per_device = list(per_device)
    p0 = per_device[0]
    arr = (C.c_void_p * len(per_device))(*[p._h for p in per_device])
    tally = C.create_string_buffer(64 * p0.n_options) if with_tally else None
    fn = getattr(_load(), f"eg_verify_{p0._prefix}_batch_multi")
    _check(fn(arr, len(per_device), n, ballots_ptr, status_ptr, tally))
    return tally.raw if with_tally else None


def verify_batch_multi_device(per_device, counts, d_ballots, d_status, streams=None, with_tally: bool = False):
    """``eg_verify_*_batch_multi_device``: slab d (counts[d] ballots at device pointer d_ballots[d], verdicts to d_status[d]) is already
    resident on the GPU of per_device[d]; streams[d] a stream of that device (None: the null streams).  Returns when every verdict is
    written; with_tally: the tally of this call's batch alone (the running tallies advance either way)."""
    per_device = list(per_device)
    p0, k = per_device[0], len(per_device)
    if any(type(p) is not type(p0) for p in per_device):
        raise ValueError("params objects of different kinds")
    if not (len(counts) == len(d_ballots) == len(d_status) == k) or (streams is not None and len(streams) != k):
        raise ValueError("one count, ballot pointer, status pointer (and stream) per params object")
    arr = (C.c_void_p * k)(*[p._h for p in per_device])
    cnt = (C.c_size_t * k)(*counts)
    db = (C.c_void_p * k)(*d_ballots)
    ds = (C.c_void_p * k)(*d_status)
    ss = (C.c_void_p * k)(*streams) if streams is not None else None
    tally = C.create_string_buffer(64 * p0.n_options) if with_tally else None
    fn = getattr(_load(), f"eg_verify_{p0._prefix}_batch_multi_device")
    _check(fn(arr, k, cnt, db, ds, ss, tally))
    return tally.raw if with_tally else None


def verify_json_multi_into(per_device, data: bytes, status, threads: int = 0, tally=None) -> int:
    """``eg_verify_*_json_multi`` with caller-owned buffers (status: ctypes uint32 array): ONE parser, the packed windows dealt to the
    params objects (one per GPU), verdicts in text order.  Returns the object count."""
    per_device = list(per_device)
    p0 = per_device[0]
    arr = (C.c_void_p * len(per_device))(*[p._h for p in per_device])
    n = sz_t(0)
    fn = getattr(_load(), f"eg_verify_{p0._prefix}_json_multi")
    _check(fn(arr, len(per_device), data, len(data), threads or effective_cores(), len(status), status, C.byref(n), tally))
    return n.value


def verify_json_multi(per_device, text, max_objects: int = 0, threads: int = 0, with_tally: bool = True):
    """JSON text -> (status words in text order, tally of this call) over several params objects of one election."""
    per_device = list(per_device)
    data = text.encode() if isinstance(text, str) else bytes(text)
    if not max_objects:
        max_objects = data.count(b"{") + 1
    st = (C.c_uint32 * max(max_objects, 1))()
    tally = C.create_string_buffer(64 * per_device[0].n_options) if with_tally else None
    n = verify_json_multi_into(per_device, data, st, threads, tally)
    return list(st[:n]), (tally.raw if with_tally else None)


def json_stream_multi(per_device, threads: int = 0) -> "JsonStream":
    """``eg_verify_*_json_begin_multi``: a JSON stream over several params objects (feed / take / end / abort as for one)."""
    return JsonStream(list(per_device), threads)


def tally_encode_multi(per_device) -> bytes:
    """Sum of the running tallies of several params objects of one election (``eg_*_tally_encode_multi``)."""
    per_device = list(per_device)
    p0 = per_device[0]
    arr = (C.c_void_p * len(per_device))(*[p._h for p in per_device])
    out = C.create_string_buffer(64 * p0.n_options)
    _check(getattr(_load(), f"eg_{p0._prefix}_tally_encode_multi")(arr, len(per_device), out))
    return out.raw


class JsonStream:
    """``eg_verify_*_json_begin / eg_verify_json_feed / _take / _end / _abort``: the JSON text of a batch of ballots in pieces of any size
    (a ballot may straddle pieces); verdicts and tally are those of ``verify_json`` on the concatenated text.  Between begin and
    end / abort the params object belongs to the stream."""

    def __init__(self, params, threads: int = 0):
        import weakref

        self._h = C.c_void_p()
        self.objects = 0
        if isinstance(params, (list, tuple)):           # several params objects of one election (one per GPU): eg_verify_*_json_begin_multi
            self.params, self.all_params = params[0], list(params)
            arr = (C.c_void_p * len(params))(*[p._h for p in params])
            fn = getattr(_load(), f"eg_verify_{params[0]._prefix}_json_begin_multi")
            _check(fn(arr, len(params), threads or effective_cores(), C.byref(self._h)))
            for p in params:                            # a params object that is destroyed takes the whole stream with it
                if not hasattr(p, "_streams"):
                    p._streams = weakref.WeakSet()
                p._streams.add(self)
        else:
            self.params, self.all_params = params, [params]
            fn = getattr(_load(), f"eg_verify_{params._prefix}_json_begin")
            _check(fn(params._h, threads or effective_cores(), C.byref(self._h)))

    def feed(self, piece) -> int:
        """The next piece of the text (bytes / bytearray / memoryview / str); returns the number of complete objects seen so far."""
        if isinstance(piece, str):
            piece = piece.encode()
        piece = bytes(piece)
        n = C.c_size_t(0)
        _check(_load().eg_verify_json_feed(self._h, C.cast(C.c_char_p(piece), C.c_void_p), len(piece), C.byref(n)))
        self.objects = n.value
        return n.value

    def feed_ptr(self, ptr: int, length: int) -> int:
        n = C.c_size_t(0)
        _check(_load().eg_verify_json_feed(self._h, C.c_void_p(ptr), length, C.byref(n)))
        self.objects = n.value
        return n.value

    def feed_owned_ptr(self, ptr: int, length: int) -> int:
        """``eg_verify_json_feed_owned``: the library reads the block at `ptr` in place - no copy on this thread, no wait for the worker -
        until the stream has been ended or aborted; the CALLER keeps the memory alive until then (the release function is the library's own
        eg_json_release_count: released_blocks() says how many blocks have come back)."""
        n = C.c_size_t(0)
        lib = _load()
        _check(lib.eg_verify_json_feed_owned(self._h, C.c_void_p(ptr), length, C.cast(lib.eg_json_release_count, C.c_void_p), C.byref(_released_blocks),
                                             C.byref(n)))
        self.objects = n.value
        return n.value

    def take(self, cap: int = 1 << 20):
        """Verdicts that are final so far (in order, from where the last take stopped).  Never waits for the GPU to drain, but it does take
        the context's lock: it may wait for the worker to finish the window of the piece it is cutting, which - while the staging ring is
        full - includes the worker's own wait for the oldest submission (include/eg_hip.h, `take`)."""
        st = (C.c_uint32 * max(cap, 1))()
        n = C.c_size_t(0)
        _check(_load().eg_verify_json_take(self._h, st, cap, C.byref(n)))
        return list(st[: n.value])

    def end(self, with_tally: bool = True, cap: int | None = None):
        """Flushes the stream: (verdicts not yet taken, tally of the stream's ballots or None).  The stream is gone afterwards."""
        cap = self.objects + 1024 if cap is None else cap
        tally = C.create_string_buffer(64 * self.params.n_options) if with_tally else None
        h, self._h = self._h, None
        while True:
            st = (C.c_uint32 * max(cap, 1))()
            n, total = C.c_size_t(0), C.c_size_t(0)
            rc = _load().eg_verify_json_end(h, st, cap, C.byref(n), C.byref(total), tally)
            if not (rc and n.value > cap):
                break
            cap = n.value                      # the stream is still open (and flushed): it had cut more objects than feed() had reported yet
        _check(rc)
        self.objects = total.value
        return list(st[: n.value]), (tally.raw if with_tally else None)

    def end_into(self, status, with_tally: bool = False):
        """As end(), verdicts into a caller-owned ctypes uint32 array (bench.py: no Python list of a million words)."""
        n, total = C.c_size_t(0), C.c_size_t(0)
        tally = C.create_string_buffer(64 * self.params.n_options) if with_tally else None
        h, self._h = self._h, None
        rc = _load().eg_verify_json_end(h, status, len(status), C.byref(n), C.byref(total), tally)
        if rc and n.value > len(status):
            self._h = h                        # no room for the n.value verdicts that are left: the stream is still open
        _check(rc)
        self.objects = total.value
        return n.value, (tally.raw if with_tally else None)

    def abort(self):
        h, self._h = getattr(self, "_h", None), None
        # a params object that has been destroyed took its open stream with it (eg_*_params_destroy aborts it): the handle is stale then
        if h and all(getattr(p, "_h", None) for p in self.all_params):
            _load().eg_verify_json_abort(h)

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


class _BatchParams:
    _prefix = ""

    def json_stream(self, threads: int = 0) -> JsonStream:
        import weakref

        st = JsonStream(self, threads)
        if not hasattr(self, "_streams"):
            self._streams = weakref.WeakSet()
        self._streams.add(st)
        return st

    def _forget_streams(self):
        """The library aborts a stream that is still open when its params object is destroyed: the Python handles must not outlive it."""
        for st in list(getattr(self, "_streams", ())):
            st._h = None

    def _fn(self, name):
        return getattr(_load(), f"eg_{self._prefix}_{name}")

    def verify_batch(self, ballots: bytes, with_tally: bool = True):
        """verify() for every packed ballot; returns (status words, tally bytes or None).
        The returned tally is that of THIS batch: the component-wise sum of the ciphertexts of its accepted ballots,
        n_options x (R || B).  The running tally inside the params object accumulates them as well, exactly as
        verify_batch_device does (tally_reset / tally_add / tally_encode operate on the running tally)."""
        n = len(ballots) // self.ballot_size
        if n * self.ballot_size != len(ballots):
            raise ValueError("ballots is not a whole number of packed ballots")
        st = (C.c_uint32 * max(n, 1))()
        tally = C.create_string_buffer(64 * self.n_options) if with_tally else None
        buf = (C.c_char * max(len(ballots), 1)).from_buffer_copy(ballots or b"\0")
        fn = getattr(_load(), f"eg_verify_{self._prefix}_batch")
        _check(fn(self._h, n, buf, st, tally))
        return list(st[:n]), (tally.raw if with_tally else None)

    def verify_json(self, text, max_objects: int = 0, threads: int = 0, with_tally: bool = True):
        """JSON text (serde's layout; one array or objects back to back) -> (status words, tally of this call) through the
        native entry point: host threads pack piece k+1 while the GPU verifies piece k.  Objects that do not deserialise get
        MALFORMED; objects of another shape than the election's get the reference's verdict (OptionsLenMismatch / LenMismatch in
        verify()'s order) from the library's object path."""
        data = text.encode() if isinstance(text, str) else bytes(text)
        if not threads:
            threads = effective_cores()
        if not max_objects:
            max_objects = data.count(b"{") + 1
        st = (C.c_uint32 * max(max_objects, 1))()
        n = sz_t(0)
        tally = C.create_string_buffer(64 * self.n_options) if with_tally else None
        fn = getattr(_load(), f"eg_verify_{self._prefix}_json")
        _check(fn(self._h, data, len(data), threads, max_objects, st, C.byref(n), tally))
        return list(st[: n.value]), (tally.raw if with_tally else None)

    def verify_json_into(self, data: bytes, status, threads: int, tally=None) -> int:
        """The same with caller-owned buffers (status: ctypes uint32 array): the bare C call, for timing.  Returns the object count."""
        n = sz_t(0)
        fn = getattr(_load(), f"eg_verify_{self._prefix}_json")
        _check(fn(self._h, data, len(data), threads, len(status), status, C.byref(n), tally))
        return n.value

    def verify_batch_host_ptr(self, n: int, ballots_ptr: int, status_ptr: int, tally_ptr: int = 0):
        """The host-buffer entry point on raw host addresses (e.g. pinned torch tensors): no Python-side copies."""
        fn = getattr(_load(), f"eg_verify_{self._prefix}_batch")
        _check(fn(self._h, n, ballots_ptr, status_ptr, tally_ptr or None))

    def verify_batch_device(self, n: int, d_ballots: int, d_status: int, stream: int = 0):
        """Asynchronous device-pointer variant (torch tensors' data_ptr()); tally accumulates on the device."""
        fn = getattr(_load(), f"eg_verify_{self._prefix}_batch_device")
        _check(fn(self._h, n, d_ballots, d_status, stream))

    def verify_small(self, ballots: bytes, with_tally: bool = True):
        """verify_batch for a handful of ballots (at most SMALL_BATCH_MAX) with low latency: one workgroup per ballot in one launch
        (eg_verify_*_small).  Same results, same running tally; returns (status words, tally of this call or None)."""
        n = len(ballots) // self.ballot_size
        if n * self.ballot_size != len(ballots):
            raise ValueError("ballots is not a whole number of packed ballots")
        st = (C.c_uint32 * max(n, 1))()
        tally = C.create_string_buffer(64 * self.n_options) if with_tally else None
        buf = (C.c_char * max(len(ballots), 1)).from_buffer_copy(ballots or b"\0")
        fn = getattr(_load(), f"eg_verify_{self._prefix}_small")
        _check(fn(self._h, n, buf, st, tally))
        return list(st[:n]), (tally.raw if with_tally else None)

    def verify_small_device(self, n: int, d_ballots: int, d_status: int, stream: int = 0):
        """Asynchronous device-pointer variant of verify_small; the tally accumulates on the device."""
        fn = getattr(_load(), f"eg_verify_{self._prefix}_small_device")
        _check(fn(self._h, n, d_ballots, d_status, stream))

    def prepare_wide_tables(self):
        """Build the wide fixed-base comb tables now instead of inside the first large verify call (eg_*_prepare_wide_tables)."""
        _check(self._fn("prepare_wide_tables")(self._h))

    def tally_reset(self, stream: int = 0):
        if stream:
            _check(self._fn("tally_reset_async")(self._h, stream))
        else:
            _check(self._fn("tally_reset")(self._h))

    def tally_encode_device(self, d_out: int, stream: int = 0):
        """Canonical encodings of the running tally (n_options x 64 bytes) into device memory, asynchronously."""
        _check(self._fn("tally_encode_device")(self._h, d_out, stream))

    def tally_add(self, encoded: bytes):
        """running tally += an encoded tally (checkpoint / resume, merging batches verified elsewhere)."""
        if len(encoded) != 64 * self.n_options:
            raise ValueError("encoded tally must be n_options x 64 bytes")
        _check(self._fn("tally_add")(self._h, encoded))

    def tally_encode(self) -> bytes:
        out = C.create_string_buffer(64 * self.n_options)
        _check(self._fn("tally_encode")(self._h, out))
        return out.raw

    def tally_grouped_scratch_bytes(self, n: int, n_groups: int) -> int:
        """Device scratch that tally_grouped_device needs for n ballots in n_groups groups (0 for arguments it refuses)."""
        return int(self._fn("tally_grouped_scratch_bytes")(self._h, n, n_groups))

    def tally_grouped(self, ballots: bytes, status, groups, n_groups: int):
        """Per-group tally of the accepted ballots of a verified batch (eg_*_tally_grouped): `status` = the words a verify entry wrote
        for `ballots`, `groups` = one group id per ballot (GROUP_NONE: in no group).  Returns (tallies, counts): tallies = n_groups x
        n_options x 64 bytes, tallies[g] what tally_encode() would give after verifying only group g's ballots; counts[g] = accepted
        ballots of group g.  Stateless: the running tally is not touched.  An accepted ballot with an id out of range, or with a
        tally point that does not decode, fails the call (EG_ERR_BAD_ARG)."""
        n = len(ballots) // self.ballot_size
        if n * self.ballot_size != len(ballots):
            raise ValueError("ballots is not a whole number of packed ballots")
        status, groups = list(status), list(groups)
        if len(status) != n or len(groups) != n:
            raise ValueError("status and groups need one word per ballot")
        st = (C.c_uint32 * max(n, 1))(*status)
        gr = (C.c_uint32 * max(n, 1))(*groups)
        buf = (C.c_char * max(len(ballots), 1)).from_buffer_copy(ballots or b"\0")
        ng = max(int(n_groups), 0)
        if not 0 < ng <= TALLY_GROUPS_MAX:                     # refused by the library: no output buffers of that size are made
            _check(self._fn("tally_grouped")(self._h, n, buf, st, gr, ng & 0xFFFFFFFF, None, None))
            raise EgError("eg_*_tally_grouped accepted a group count it must refuse")
        tallies = C.create_string_buffer(ng * 64 * self.n_options)
        counts = (C.c_uint32 * ng)()
        _check(self._fn("tally_grouped")(self._h, n, buf, st, gr, ng, tallies, counts))
        return tallies.raw, list(counts)

    def tally_grouped_device(self, n: int, d_ballots: int, d_status: int, d_groups: int, n_groups: int, d_scratch: int, d_tallies: int,
                             d_bad: int, d_counts: int = 0, stream: int = 0):
        """Asynchronous device-pointer variant (eg_*_tally_grouped_device): no allocation, no host synchronisation.  d_scratch:
        tally_grouped_scratch_bytes(n, n_groups) bytes; d_bad: two uint32 the library writes (ids out of range, undecodable points) -
        the caller must read them and discard the tallies if either is non-zero."""
        _check(self._fn("tally_grouped_device")(self._h, n, d_ballots or None, d_status or None, d_groups or None, n_groups,
                                                 d_scratch or None, d_tallies or None, d_counts or None, d_bad or None, stream or None))

    def tally_weighted_scratch_bytes(self, n: int, n_groups: int = 1) -> int:
        """Device scratch that tally_weighted_device needs for n ballots in n_groups groups (0 for arguments it refuses)."""
        return int(self._fn("tally_weighted_scratch_bytes")(self._h, n, n_groups))

    def tally_weighted(self, ballots: bytes, status, weights, groups=None, n_groups: int = 1, weight_bits: int = 64):
        """Weighted per-group tally of the accepted ballots of a verified batch (eg_*_tally_weighted): ballot b adds weights[b] times
        its ciphertexts to the tally of groups[b] (`groups` None: one group).  weights[b] < 2**weight_bits <= 2**64; weight_bits fixes
        the cost per point, so pass the smallest bound that holds.  Returns (tallies, weight_sums, counts): tallies as tally_grouped,
        weight_sums[g] = the exact sum of the counted weights of group g (a Python int, the bound for DlogSolver.solve), counts[g] =
        its accepted ballots.  Stateless.  A stray group id, a tally point that does not decode or a weight of 2**weight_bits or more
        on an accepted ballot fails the call (EG_ERR_BAD_ARG)."""
        n = len(ballots) // self.ballot_size
        if n * self.ballot_size != len(ballots):
            raise ValueError("ballots is not a whole number of packed ballots")
        status, weights = list(status), list(weights)
        if len(status) != n or len(weights) != n or (groups is not None and len(groups) != n):
            raise ValueError("status, weights and groups need one word per ballot")
        if any(not 0 <= int(w) < 1 << 64 for w in weights):
            raise ValueError("a weight is outside 0 .. 2^64 - 1")
        st = (C.c_uint32 * max(n, 1))(*status)
        wt = (C.c_uint64 * max(n, 1))(*weights)
        gr = None if groups is None else (C.c_uint32 * max(n, 1))(*groups)
        buf = (C.c_char * max(len(ballots), 1)).from_buffer_copy(ballots or b"\0")
        ng = max(int(n_groups), 0)
        if not 0 < ng <= TALLY_GROUPS_MAX:                     # refused by the library: no output buffers of that size are made
            _check(self._fn("tally_weighted")(self._h, n, buf, st, wt, weight_bits, gr, ng & 0xFFFFFFFF, None, None, None))
            raise EgError("eg_*_tally_weighted accepted a group count it must refuse")
        tallies = C.create_string_buffer(ng * 64 * self.n_options)
        sums = (C.c_uint64 * (2 * ng))()
        counts = (C.c_uint32 * ng)()
        _check(self._fn("tally_weighted")(self._h, n, buf, st, wt, weight_bits, gr, ng, tallies, sums, counts))
        return tallies.raw, [sums[2 * g] | (sums[2 * g + 1] << 64) for g in range(ng)], list(counts)

    def tally_weighted_device(self, n: int, d_ballots: int, d_status: int, d_weights: int, weight_bits: int, d_groups: int, n_groups: int,
                              d_scratch: int, d_tallies: int, d_bad: int, d_weight_sums: int = 0, d_counts: int = 0, stream: int = 0):
        """Asynchronous device-pointer variant (eg_*_tally_weighted_device): no allocation, no host synchronisation.  d_weights: n
        uint64; d_groups may be 0 (one group); d_scratch: tally_weighted_scratch_bytes(n, n_groups) bytes; d_weight_sums: n_groups x
        (low, high) uint64; d_bad: three uint32 the library writes (ids out of range, undecodable points, weights out of range) - the
        caller must read them and discard the results if any is non-zero."""
        _check(self._fn("tally_weighted_device")(self._h, n, d_ballots or None, d_status or None, d_weights or None, weight_bits,
                                                  d_groups or None, n_groups, d_scratch or None, d_tallies or None, d_weight_sums or None,
                                                  d_counts or None, d_bad or None, stream or None))

    def weed_scratch_bytes(self, n: int, n_prior: int = 0) -> int:
        """Device scratch that weed_device needs for n ballots beside a board of n_prior ciphertexts (0 for arguments it refuses)."""
        return int(self._fn("weed_scratch_bytes")(self._h, n, n_prior))

    def weed(self, ballots: bytes, status=None, board: bytes = b"", append: bool = False):
        """Ballot weeding between verify and tally (eg_*_weed): flags every participating ballot (status word 0; `status` None: every
        ballot) that repeats a tally ciphertext - 64 wire bytes R || B - of `board` (ciphertexts cast in earlier batches, 64 bytes each)
        or of an earlier participating ballot of the batch.  Returns (dup_of, status_out, appended): dup_of[b] = DUP_NONE, DUP_PRIOR or
        the smallest earlier ballot that shares a ciphertext with b (it counts even if it is flagged itself); status_out = the status
        words with ST_DUPLICATE for the flagged ballots, ready for tally_grouped / tally_weighted; appended = with `append`, the
        ciphertexts of the participating, unflagged ballots in ballot and option order - what to add to the board - else None."""
        n = len(ballots) // self.ballot_size
        if n * self.ballot_size != len(ballots):
            raise ValueError("ballots is not a whole number of packed ballots")
        if len(board) % 64:
            raise ValueError("board is not a whole number of 64-byte ciphertexts")
        st = None
        if status is not None:
            status = list(status)
            if len(status) != n:
                raise ValueError("status needs one word per ballot")
            st = (C.c_uint32 * max(n, 1))(*status)
        buf = (C.c_char * max(len(ballots), 1)).from_buffer_copy(ballots or b"\0")
        brd = (C.c_char * max(len(board), 1)).from_buffer_copy(board or b"\0")
        dup, out = (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
        app = C.create_string_buffer(max(n * self.n_options * 64, 1)) if append else None
        n_app = sz_t(0)
        _check(self._fn("weed")(self._h, n, buf, st, len(board) // 64, brd, dup, out, app, C.byref(n_app)))
        return list(dup[:n]), list(out[:n]), (app.raw[: 64 * n_app.value] if append else None)

    def weed_device(self, n: int, d_ballots: int, d_status: int, n_prior: int, d_board: int, board_cap: int, hash_seed: int, d_scratch: int,
                    d_dup_of: int, d_found: int, d_status_out: int = 0, d_board_count: int = 0, stream: int = 0):
        """Asynchronous device-pointer variant (eg_*_weed_device): no allocation, no host synchronisation, no lock.  d_status may be 0
        (every ballot participates); d_board: board_cap x 64 bytes of which the first n_prior are the board; hash_seed: 64 random bits,
        fresh per call and unpublished until it is over; d_scratch: weed_scratch_bytes(n, n_prior) bytes; d_dup_of: n uint32;
        d_status_out may be 0 or d_status; d_board_count: one uint64, 0 = do not append; d_found: three uint32 the library writes
        (flagged against the board, flagged against the batch, the bad word - discard the results if it is non-zero)."""
        _check(self._fn("weed_device")(self._h, n, d_ballots or None, d_status or None, n_prior, d_board or None, board_cap,
                                        hash_seed & 0xFFFFFFFFFFFFFFFF, d_scratch or None, d_dup_of or None, d_status_out or None,
                                        d_board_count or None, d_found or None, stream or None))

    def weed_indexed_scratch_bytes(self, n: int) -> int:
        """Device scratch that weed_indexed_device needs for n ballots: a function of n alone, whatever the board's size (0 for arguments
        it refuses)."""
        return int(self._fn("weed_indexed_scratch_bytes")(self._h, n))

    def weed_indexed_device(self, n: int, d_ballots: int, d_status: int, n_prior: int, d_board: int, board_cap: int, d_index: int,
                            index_seed: int, hash_seed: int, d_scratch: int, d_dup_of: int, d_found: int, d_status_out: int = 0,
                            d_board_count: int = 0, stream: int = 0):
        """weed_device against a persistent board index (eg_*_weed_indexed_device): the same outputs byte for byte at O(batch) per call.
        d_index: Context.weed_index_bytes(board_cap) bytes, built by Context.weed_index_build_device over board [0, n_prior) with
        index_seed and maintained by earlier calls; with d_board_count the appended ciphertexts are added to it, without it is only read.
        index_seed stays unpublished for the life of the index; hash_seed is fresh per call; d_scratch: weed_indexed_scratch_bytes(n)."""
        _check(self._fn("weed_indexed_device")(self._h, n, d_ballots or None, d_status or None, n_prior, d_board or None, board_cap,
                                                d_index or None, index_seed & 0xFFFFFFFFFFFFFFFF, hash_seed & 0xFFFFFFFFFFFFFFFF,
                                                d_scratch or None, d_dup_of or None, d_status_out or None, d_board_count or None,
                                                d_found or None, stream or None))

    def open_check_scratch_bytes(self, n: int) -> int:
        """Device scratch that open_check_device needs for n opened ballots (0 for arguments it refuses)."""
        return int(self._fn("open_check_scratch_bytes")(self._h, n))

    def open_check(self, ballots: bytes, values, rand: bytes, status_in=None):
        """Ballot audit (eg_*_open_check; include/eg_hip.h, "ballot audits" has the rule): do the opened ballots encrypt what their
        openings say.  values = n x n_options integers below 2**64 and rand = n x n_options x 32 bytes, the value and the encryption
        randomness of every tally ciphertext in ballot and then slot order.  Returns (status_out, found): status_out[b] = 0, the word
        of status_in for a ballot that does not participate, or ST_BAD_OPENING with open_detail(slot, check) as its detail; found =
        [ballots that participated, ballots that failed].  An opened ballot must never be counted: put its ciphertexts onto
        weeding's board (weed(..., append=True) over the audited pile)."""
        n = len(ballots) // self.ballot_size
        if n * self.ballot_size != len(ballots):
            raise ValueError("ballots is not a whole number of packed ballots")
        values = list(values)
        if len(values) != n * self.n_options or len(rand) != 32 * n * self.n_options:
            raise ValueError("values and rand need one entry per ballot and option")
        if any(not 0 <= int(v) < 1 << 64 for v in values):
            raise ValueError("a value is outside 0 .. 2^64 - 1")
        sin = None
        if status_in is not None:
            status_in = list(status_in)
            if len(status_in) != n:
                raise ValueError("status_in needs one word per ballot")
            sin = (C.c_uint32 * max(n, 1))(*status_in)
        buf = (C.c_char * max(len(ballots), 1)).from_buffer_copy(ballots or b"\0")
        val = (C.c_uint64 * max(len(values), 1))(*values)
        rnd = (C.c_char * max(len(rand), 1)).from_buffer_copy(rand or b"\0")
        out, found = (C.c_uint32 * max(n, 1))(), (C.c_uint32 * 2)()
        _check(self._fn("open_check")(self._h, n, buf, sin, val, rnd, out, found))
        return list(out[:n]), list(found)

    def open_check_device(self, n: int, d_ballots: int, d_values: int, d_rand: int, d_status_out: int, d_found: int, d_scratch: int,
                          d_status_in: int = 0, stream: int = 0):
        """Asynchronous device-pointer variant (eg_*_open_check_device): no allocation, no host synchronisation, no lock.  d_values: n x
        n_options uint64; d_rand: n x n_options x 32 bytes; d_status_out: n uint32, may be d_status_in; d_found: two uint32 the
        library writes; d_scratch: open_check_scratch_bytes(n) bytes."""
        _check(self._fn("open_check_device")(self._h, n, d_ballots or None, d_status_in or None, d_values or None, d_rand or None,
                                              d_status_out or None, d_found or None, d_scratch or None, stream or None))

    def _open_batch(self, n: int, call):
        values = (C.c_uint64 * max(n * self.n_options, 1))()
        rand = C.create_string_buffer(max(32 * n * self.n_options, 1))
        _check(call(values, rand))
        return list(values[: n * self.n_options]), rand.raw[: 32 * n * self.n_options]


class ChoiceParams(_BatchParams):
    """``ChoiceParams::single(pk, n)`` / ``::multi(pk, n)`` (choice.rs:160-196)."""

    _prefix = "choice"

    def __init__(self, ctx: Context, public_key: bytes, options_count: int, single: bool = True):
        self.ctx, self.public_key, self.n_options, self.single = ctx, public_key, options_count, single
        self._h = C.c_void_p()
        _check(_load().eg_choice_params_create(ctx._h, public_key, options_count, int(single), C.byref(self._h)))
        self.ballot_size = _load().eg_choice_ballot_size(options_count, int(single))

    @property
    def kind_name(self) -> str:
        """The name plan_describe() knows this election's plan by."""
        return "single" if self.single else "multi"

    @classmethod
    def single_choice(cls, ctx, public_key, options_count):
        return cls(ctx, public_key, options_count, True)

    @classmethod
    def multi_choice(cls, ctx, public_key, options_count):
        return cls(ctx, public_key, options_count, False)

    def encrypt_batch(self, base_seed: int, first: int, n: int, n_selected: int = 0) -> bytes:
        """EncryptedChoice::new for n synthetic voters (GPU), returned packed in host memory."""
        out = C.create_string_buffer(max(n * self.ballot_size, 1))
        _check(_load().eg_choice_encrypt_batch(self._h, base_seed, first, n, n_selected, out))
        return out.raw[: n * self.ballot_size]

    def encrypt_batch_device(self, base_seed: int, first: int, n: int, d_out: int, n_selected: int = 0, stream: int = 0):
        """EncryptedChoice::new for n synthetic voters, written packed to device memory."""
        _check(_load().eg_choice_encrypt_batch_device(self._h, base_seed, first, n, n_selected, d_out, stream))

    def encrypt_selected(self, base_seed: int, first: int, selections, rng_skip: int = 0) -> bytes:
        """``EncryptedChoice::single(params, choice, rng)`` / ``::new(params, &[bool], rng)`` (choice.rs:296-349) on the GPU for the
        caller's choices: `selections` = one bitmask per ballot (bit k <=> option k chosen); ballot i uses
        ChaChaRng::seed_from_u64(base_seed + first + i) after `rng_skip` 64-byte draws.  Returns the packed ballots."""
        sel = list(selections)
        n = len(sel)
        sw = (self.n_options + 31) // 32                       # bitmask words per ballot
        words = [(int(m) >> (32 * w)) & 0xFFFFFFFF for m in sel for w in range(sw)]
        arr = (C.c_uint32 * max(len(words), 1))(*words)
        out = C.create_string_buffer(max(n * self.ballot_size, 1))
        _check(_load().eg_choice_encrypt_selected_batch(self._h, base_seed, first, n, rng_skip, arr, out))
        return out.raw[: n * self.ballot_size]

    def open_batch(self, base_seed: int, first: int, n: int, selections=None, rng_skip: int = 0, n_selected: int = 0):
        """The opener (eg_choice_open_batch; VARIABLE TIME, test and benchmark openings only): (values, rand) of the ballots that
        encrypt_selected(base_seed, first, selections, rng_skip) makes or, with `selections` None, encrypt_batch(base_seed, first, n,
        n_selected) (rng_skip 0).  values = n x n_options integers (1 = chosen), rand = n x n_options x 32 bytes."""
        arr = None
        if selections is not None:
            sel = list(selections)
            if len(sel) != n:
                raise ValueError("selections needs one bitmask per ballot")
            sw = (self.n_options + 31) // 32
            words = [(int(m) >> (32 * w)) & 0xFFFFFFFF for m in sel for w in range(sw)]
            arr = (C.c_uint32 * max(len(words), 1))(*words)
        return self._open_batch(n, lambda v, r: _load().eg_choice_open_batch(self._h, base_seed, first, n, n_selected, rng_skip, arr, v, r))

    def open_batch_device(self, base_seed: int, first: int, n: int, d_values_out: int, d_rand_out: int, d_selection: int = 0,
                          rng_skip: int = 0, n_selected: int = 0, stream: int = 0):
        """The opener on device buffers (eg_choice_open_batch_device): asynchronous on `stream`, no lock, no workspace."""
        _check(_load().eg_choice_open_batch_device(self._h, base_seed, first, n, n_selected, rng_skip, d_selection or None,
                                                   d_values_out or None, d_rand_out or None, stream or None))

    def close(self):
        if getattr(self, "_h", None):
            _load().eg_choice_params_destroy(self._h)
            self._forget_streams()
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PublicKeyVerifier:
    """Batched ``PublicKey::verify_zero / verify_bool / verify_range`` (src/keys/impls.rs:59-69,100-112,142-151)."""

    ZERO, BOOL, RANGE = 0, 1, 2
    _value_rows = False      # prove() takes one value per item (a sum of squares: one row of values)

    def __init__(self, ctx: Context, public_key: bytes, kind: int, upper_bound: int = 0):
        self.ctx, self.kind = ctx, kind
        self._h = C.c_void_p()
        _check(_load().eg_proof_params_create(ctx._h, public_key, kind, upper_bound, C.byref(self._h)))
        self.item_size = _load().eg_proof_item_size(self._h)

    def verify_batch(self, items: bytes):
        n = len(items) // self.item_size
        if n * self.item_size != len(items):
            raise ValueError("items is not a whole number of packed proofs")
        st = (C.c_uint32 * max(n, 1))()
        buf = (C.c_char * max(len(items), 1)).from_buffer_copy(items or b"\0")
        _check(_load().eg_verify_proof_batch(self._h, n, buf, st))
        return list(st[:n])

    def verify_device(self, n: int, d_items: int, d_status: int, stream: int = 0):
        """n items at device pointer d_items -> n status words (uint32) at d_status; asynchronous on `stream`."""
        _check(_load().eg_verify_proof_batch_device(self._h, n, d_items, d_status, stream))

    def prove(self, base_seed: int, first: int, values_or_n, rng_skip: int = 0) -> bytes:
        """``PublicKey::encrypt_zero / encrypt_bool / encrypt_range`` and ``SumOfSquaresProof::new`` on the GPU (test and benchmark
        inputs: variable time); item i draws from ChaChaRng::seed_from_u64(base_seed + first + i) after `rng_skip` 64-byte draws.
        `values_or_n`: the number of items for ZERO; one value per item for BOOL (0 / 1 / bool) and RANGE; one sequence of n_values
        integers per item for a sum of squares.  Returns the packed items, as `verify_batch` takes them."""
        per = _load().eg_proof_prove_input_size(self._h) // 8
        if per == 0:
            n, arr = int(values_or_n), None
        else:
            rows = list(values_or_n)
            n = len(rows)
            flat = [int(x) for row in rows for x in row] if self._value_rows else [int(v) for v in rows]
            if len(flat) != n * per:
                raise ValueError(f"every item needs {per} values")
            arr = (C.c_uint64 * max(len(flat), 1))(*flat)
        out = C.create_string_buffer(max(n * self.item_size, 1))
        _check(_load().eg_proof_prove_batch(self._h, base_seed, first, n, rng_skip, arr, out))
        return out.raw[: n * self.item_size]

    def prove_device(self, base_seed: int, first: int, n: int, d_inputs: int, d_items: int, rng_skip: int = 0, stream: int = 0):
        """The same on device buffers: the items' uint64 inputs at d_inputs (0 for ZERO) -> n items at d_items; asynchronous on
        `stream`.  The inputs are trusted."""
        _check(_load().eg_proof_prove_batch_device(self._h, base_seed, first, n, rng_skip, d_inputs or None, d_items, stream))

    def close(self):
        if getattr(self, "_h", None):
            _load().eg_proof_params_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SumOfSquaresVerifier(PublicKeyVerifier):
    """Batched ``SumOfSquaresProof::verify`` (src/proofs/mul.rs:190-260) with ``Transcript::new(label)``.
    item = n value ciphertexts || sum-of-squares ciphertext || challenge || 2n ciphertext responses || sum response."""

    _value_rows = True

    def __init__(self, ctx: Context, public_key: bytes, n_values: int, label: bytes):
        self.ctx, self.kind = ctx, 4
        self._h = C.c_void_p()
        _check(_load().eg_sumsq_params_create(ctx._h, public_key, n_values, label, len(label), C.byref(self._h)))
        self.item_size = _load().eg_proof_item_size(self._h)


class CommitmentEquivalenceVerifier(PublicKeyVerifier):
    """Batched ``CommitmentEquivalenceProof::verify`` (src/proofs/commitment.rs:186-238) with ``Transcript::new(label)``: the ElGamal
    ciphertext (R, B) under `public_key` and the Pedersen commitment C = [v]G + [r_c]H over `blinding_base` H hide the same value.
    item (224 bytes) = R || B || C || challenge || randomness_response || value_response || commitment_response
    (serde.pack_commitment_equivalence packs the reference's object).  H must not be the identity."""

    ITEM_SIZE = 224

    def __init__(self, ctx: Context, public_key: bytes, blinding_base: bytes, label: bytes):
        self.ctx, self.kind = ctx, 5
        self.public_key, self.blinding_base, self.label = public_key, blinding_base, label
        if len(public_key) != 32 or len(blinding_base) != 32:
            raise ValueError("public_key and blinding_base are 32-byte encodings")
        self._h = C.c_void_p()
        _check(_load().eg_commit_equiv_params_create(ctx._h, public_key, blinding_base, label, len(label), C.byref(self._h)))
        self.item_size = _load().eg_proof_item_size(self._h)

    def verify(self, items: bytes):
        """Status words of the packed items (host memory)."""
        return self.verify_batch(items)

    def prove(self, base_seed: int, first: int, values, rng_skip: int = 0, with_blindings: bool = False):
        """``CommitmentEquivalenceProof::new`` on the GPU, one item per value (test and benchmark inputs: variable time); item i draws
        from ChaChaRng::seed_from_u64(base_seed + first + i) after `rng_skip` 64-byte draws.  Returns the packed items, and the blinding
        scalars r_c (32 bytes each) as well when `with_blindings`."""
        vals = [int(v) for v in values]
        n = len(vals)
        arr = (C.c_uint64 * max(n, 1))(*vals)
        out = C.create_string_buffer(max(n * self.item_size, 1))
        bl = C.create_string_buffer(max(n * 32, 1)) if with_blindings else None
        _check(_load().eg_commit_equiv_prove_batch(self._h, base_seed, first, n, rng_skip, arr, out, bl))
        items = out.raw[: n * self.item_size]
        return (items, bl.raw[: n * 32]) if with_blindings else items

    def prove_device(self, base_seed: int, first: int, n: int, d_values: int, d_items: int, d_blindings: int = 0, rng_skip: int = 0,
                     stream: int = 0):
        """The same on device buffers: n uint64 values at d_values -> n items at d_items (and n x 32 bytes of r_c at d_blindings
        unless 0); asynchronous on `stream`."""
        _check(_load().eg_commit_equiv_prove_batch_device(self._h, base_seed, first, n, rng_skip, d_values, d_items,
                                                          d_blindings or None, stream))


class DecryptionShareVerifier(PublicKeyVerifier):
    """Batched ``PublicKeySet::verify_share`` for one participant (src/sharing/key_set.rs:209-228).
    item = ciphertext.random_element || dh_element || challenge || response."""

    def __init__(self, ctx: Context, shared_key: bytes, shares: int, threshold: int, index: int, participant_key: bytes):
        self.ctx, self.kind = ctx, 3
        self._h = C.c_void_p()
        _check(_load().eg_share_params_create(ctx._h, shared_key, shares, threshold, index, participant_key, C.byref(self._h)))
        self.item_size = _load().eg_proof_item_size(self._h)

    def prove(self, secret_share: bytes, base_seed: int, first: int, ct_randoms: bytes, rng_skip: int = 0):
        """``ActiveParticipant::decrypt_share`` on the GPU for this participant (test and benchmark inputs: variable time in the secret
        share): one item per 32-byte random element of `ct_randoms`, item i drawing from ChaChaRng::seed_from_u64(base_seed + first + i)
        after `rng_skip` 64-byte draws.  Returns (packed items, ok bytes); an element that does not decode gets ok 0 and a zeroed item."""
        if len(secret_share) != 32 or len(ct_randoms) % 32:
            raise ValueError("secret_share and every random element are 32-byte encodings")
        n = len(ct_randoms) // 32
        out = C.create_string_buffer(max(n * self.item_size, 1))
        ok = C.create_string_buffer(max(n, 1))
        buf = (C.c_char * max(len(ct_randoms), 1)).from_buffer_copy(ct_randoms or b"\0")
        _check(_load().eg_share_prove_batch(self._h, secret_share, base_seed, first, n, rng_skip, buf, out, ok))
        return out.raw[: n * self.item_size], ok.raw[:n]

    def prove_device(self, secret_share: bytes, base_seed: int, first: int, n: int, d_ct_randoms: int, d_items: int, d_ok: int,
                     rng_skip: int = 0, stream: int = 0):
        """The same on device buffers: n x 32 bytes at d_ct_randoms -> n items at d_items and n ok bytes at d_ok; asynchronous on
        `stream`.  The secret share is trusted to be canonical."""
        _check(_load().eg_share_prove_batch_device(self._h, secret_share, base_seed, first, n, rng_skip, d_ct_randoms, d_items, d_ok,
                                                   stream))


class QuadraticVotingParams(_BatchParams):
    """``QuadraticVotingParams::new(pk, options, credits)`` (quadratic_voting.rs:63-76)."""

    _prefix = "qv"
    kind_name = "qv"

    def __init__(self, ctx: Context, public_key: bytes, options_count: int, credits: int):
        self.ctx, self.public_key, self.n_options, self.credits = ctx, public_key, options_count, credits
        self._h = C.c_void_p()
        _check(_load().eg_qv_params_create(ctx._h, public_key, options_count, credits, C.byref(self._h)))
        self.ballot_size = _load().eg_qv_ballot_size(self._h)

    def encrypt_batch_device(self, base_seed: int, first: int, n: int, d_out: int, stream: int = 0):
        """QuadraticVotingBallot::new for n synthetic voters, written packed to device memory."""
        _check(_load().eg_qv_encrypt_batch_device(self._h, base_seed, first, n, d_out, stream))

    def encrypt_votes(self, base_seed: int, first: int, votes, rng_skip: int = 0) -> bytes:
        """``QuadraticVotingBallot::new(params, votes, rng)`` (quadratic_voting.rs:234-284) on the GPU for the caller's votes
        (one list of n_options integers per ballot); RNG as in ChoiceParams.encrypt_selected."""
        votes = [list(v) for v in votes]
        n = len(votes)
        if any(len(v) != self.n_options for v in votes):
            raise ValueError("every ballot needs n_options votes")
        flat = [x for v in votes for x in v]
        arr = (C.c_uint32 * max(len(flat), 1))(*flat)
        out = C.create_string_buffer(max(n * self.ballot_size, 1))
        _check(_load().eg_qv_encrypt_votes_batch(self._h, base_seed, first, n, rng_skip, arr, out))
        return out.raw[: n * self.ballot_size]

    def open_batch(self, base_seed: int, first: int, n: int, votes=None, rng_skip: int = 0):
        """The opener (eg_qv_open_batch; VARIABLE TIME, test and benchmark openings only): (values, rand) of the vote ciphertexts of
        the ballots that encrypt_votes(base_seed, first, votes, rng_skip) makes or, with `votes` None, encrypt_batch_device(base_seed,
        first, n) (rng_skip 0).  values = n x n_options votes, rand = n x n_options x 32 bytes."""
        arr = None
        if votes is not None:
            votes = [list(v) for v in votes]
            if len(votes) != n or any(len(v) != self.n_options for v in votes):
                raise ValueError("every ballot needs n_options votes")
            flat = [x for v in votes for x in v]
            arr = (C.c_uint32 * max(len(flat), 1))(*flat)
        return self._open_batch(n, lambda v, r: _load().eg_qv_open_batch(self._h, base_seed, first, n, rng_skip, arr, v, r))

    def open_batch_device(self, base_seed: int, first: int, n: int, d_values_out: int, d_rand_out: int, d_votes: int = 0,
                          rng_skip: int = 0, stream: int = 0):
        """The opener on device buffers (eg_qv_open_batch_device): asynchronous on `stream`, no lock, no workspace."""
        _check(_load().eg_qv_open_batch_device(self._h, base_seed, first, n, rng_skip, d_votes or None, d_values_out or None,
                                               d_rand_out or None, stream or None))

    def close(self):
        if getattr(self, "_h", None):
            _load().eg_qv_params_destroy(self._h)
            self._forget_streams()
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
