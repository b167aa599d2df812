"""Tally stage (examples/voting.rs:122-177): combine verified decryption shares by Lagrange interpolation
in the exponent and read the vote counts off a discrete-log table.

Thin ctypes mirror of the C entry points (`eg_combine_shares[_batch]`, `eg_dlog_table_*`, `eg_dlog_solver_*`, include/eg_hip.h), which mirror
``lagrange_coefficients`` / ``Params::combine_shares`` (src/sharing/mod.rs:139-170,302-325) and ``DiscreteLogTable``
(src/encryption.rs:260-298).  All scalar and group arithmetic runs on the GPU primitives inside the library.
"""
from __future__ import annotations

import ctypes as C

from . import _check, _load


def combine_shares(group, threshold: int, shares, n_shares: int | None = None):
    """``Params::combine_shares``: shares = [(participant index, dh_element bytes)]; the first `threshold` are used.
    Returns the combined dh element [x]R, or None if there are too few shares.  `n_shares` = participants of the key set
    (default: large enough for the indexes given)."""
    shares = list(shares)
    n = len(shares)
    total = n_shares if n_shares is not None else max([i for i, _ in shares] + [threshold - 1]) + 1
    idx = (C.c_uint64 * max(n, 1))(*[i for i, _ in shares])
    out = C.create_string_buffer(32)
    combined = C.c_int(0)
    _check(_load().eg_combine_shares(group.ctx._h, total, threshold, n, idx, b"".join(s for _, s in shares), out, C.byref(combined)))
    return out.raw if combined.value else None


COMBINE_SHARES_MAX = 64      # EG_COMBINE_SHARES_MAX


def combine_shares_batch_scratch_bytes(threshold: int, m: int) -> int:
    """Device scratch that combine_shares_batch_device needs for m ciphertexts (0 for arguments it refuses)."""
    return int(_load().eg_combine_shares_batch_scratch_bytes(threshold, m))


def combine_shares_batch(group, shares: int, threshold: int, ciphertexts: bytes, indexes, items: bytes, status=None):
    """``Params::combine_shares`` and ``VerifiableDecryption::decrypt_to_element`` for a whole vector of ciphertexts in one pass
    (eg_combine_shares_batch).  ciphertexts: m x 64 bytes (R || B); indexes: the zero-based participant index of each of the k columns;
    items: k x m decryption-share items of 128 bytes, column after column (column j = participant indexes[j]'s m items, item c for
    ciphertext c); status: k x m status words as ``DecryptionShareVerifier.verify_batch`` gave them, column after column, or None for
    "every share accepted".  Per ciphertext the first `threshold` usable columns are combined.
    Returns (dh, plain, combined, used): m x 32 bytes [x]R, m x 32 bytes B - [x]R (what the discrete-log solver takes), m flags
    (0: fewer than `threshold` usable shares - the reference's None - with zero bytes in dh and plain) and m masks with bit i set for
    every participant i whose share was used.  A share marked accepted that carries another ciphertext's R, a chosen share or a B that
    does not decode fails the call (EG_ERR_BAD_ARG)."""
    indexes = [int(i) for i in indexes]
    k = len(indexes)
    if len(ciphertexts) % 64:
        raise ValueError("ciphertexts is not a whole number of 64-byte ciphertexts")
    m = len(ciphertexts) // 64
    if len(items) != k * m * 128:
        raise ValueError("items needs one 128-byte item per column and ciphertext")
    if any(not 0 <= i < 1 << 64 for i in indexes):
        raise ValueError("an index is outside 0 .. 2^64 - 1")
    st = None
    if status is not None:
        status = list(status)
        if len(status) != k * m:
            raise ValueError("status needs one word per column and ciphertext")
        st = (C.c_uint32 * max(k * m, 1))(*status)
    idx = (C.c_uint64 * max(k, 1))(*indexes)
    cts = (C.c_char * max(len(ciphertexts), 1)).from_buffer_copy(ciphertexts or b"\0")
    its = (C.c_char * max(len(items), 1)).from_buffer_copy(items or b"\0")
    dh, plain = C.create_string_buffer(max(32 * m, 1)), C.create_string_buffer(max(32 * m, 1))
    combined, used = C.create_string_buffer(max(m, 1)), (C.c_uint64 * max(m, 1))()
    h = group.ctx._h if group is not None else None
    _check(_load().eg_combine_shares_batch(h, shares, threshold, m, cts, k, idx, its, st, dh, plain, combined, used))
    return dh.raw[: 32 * m], plain.raw[: 32 * m], list(combined.raw[:m]), list(used[:m])


def combine_shares_batch_device(group, shares: int, threshold: int, m: int, d_ciphertexts: int, indexes, d_items: int, d_status: int,
                                d_combined: int, d_bad: int, d_scratch: int, d_dh: int = 0, d_plain: int = 0, d_used: int = 0,
                                stream: int = 0):
    """Asynchronous device-pointer variant (eg_combine_shares_batch_device): no allocation, no host synchronisation, no lock.
    `indexes` stay on the host; d_status may be 0 (every share accepted); d_scratch: combine_shares_batch_scratch_bytes(threshold, m)
    bytes; d_bad: three uint32 the library writes (shares of another ciphertext, chosen shares that do not decode, undecodable B) - the
    caller must read them and discard the results if any is non-zero."""
    indexes = [int(i) for i in indexes]
    idx = (C.c_uint64 * max(len(indexes), 1))(*indexes)
    h = group.ctx._h if group is not None else None
    _check(_load().eg_combine_shares_batch_device(h, shares, threshold, m, d_ciphertexts or None, len(indexes), idx, d_items or None,
                                                  d_status or None, d_dh or None, d_plain or None, d_combined or None, d_used or None,
                                                  d_bad or None, d_scratch or None, stream or None))


class DiscreteLogTable:
    """``DiscreteLogTable::new(values)``: maps [m]G (canonical encoding) back to m."""

    def __init__(self, group, values):
        values = list(values)
        arr = (C.c_uint64 * max(len(values), 1))(*values)
        self._h = C.c_void_p()
        _check(_load().eg_dlog_table_create(group.ctx._h, len(values), arr, C.byref(self._h)))

    def get(self, element: bytes):
        v, found = C.c_uint64(0), C.create_string_buffer(1)
        _check(_load().eg_dlog_table_get(self._h, 1, element, C.byref(v), found))
        return int(v.value) if found.raw[0] else None

    def close(self):
        if getattr(self, "_h", None):
            _load().eg_dlog_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decrypt_total(group, table: DiscreteLogTable, ciphertext: bytes, combined_dh: bytes):
    """``VerifiableDecryption::decrypt``: blinded_element - dh looked up in the table (None if absent)."""
    m, ok = group.element_add(ciphertext[32:64], combined_dh, subtract=True)
    return table.get(m)


class DiscreteLogSolver:
    """``DiscreteLogTable::new(lo..hi).get(e)`` for ranges no table can hold: baby-step/giant-step on the GPU over a table of
    2^baby_bits multiples of the generator, built once (0 = the library's default width).  One solver serves any range."""

    def __init__(self, group, baby_bits: int = 0):
        self._h = C.c_void_p()
        _check(_load().eg_dlog_solver_create(group.ctx._h, baby_bits, C.byref(self._h)))

    def solve(self, elements, lo: int, hi: int):
        """elements: 32-byte encodings -> [m or None]: the m in [lo, hi) with [m]G == element (the identity is always 0)."""
        elements = list(elements)
        n = len(elements)
        values, found = (C.c_uint64 * max(n, 1))(), C.create_string_buffer(max(n, 1))
        _check(_load().eg_dlog_solver_solve(self._h, n, b"".join(elements), lo, hi, values, found))
        return [int(values[i]) if found.raw[i] else None for i in range(n)]

    def max_span(self, n: int) -> int:
        """The widest hi - lo that solve() accepts for n elements."""
        return int(_load().eg_dlog_solver_max_span(self._h, n))

    @property
    def table_bytes(self) -> int:
        return int(_load().eg_dlog_solver_table_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None):
            _load().eg_dlog_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decrypt_totals(group, solver: DiscreteLogSolver, ciphertexts, combined_dhs, lo: int, hi: int):
    """``VerifiableDecryption::decrypt`` for every option of a tally at once: blinded_element - dh, then one solve over [lo, hi)."""
    ciphertexts, combined_dhs = list(ciphertexts), list(combined_dhs)
    m, ok = group.element_add(b"".join(ct[32:64] for ct in ciphertexts), b"".join(combined_dhs), subtract=True)
    return solver.solve([m[32 * i : 32 * i + 32] for i in range(len(ciphertexts))], lo, hi)


def decrypt_tallies(group, shares: int, threshold: int, ciphertexts, verifiers, items, solver=None, lo: int = 0, hi: int = 0, table=None):
    """The tally stage for a whole vector of ciphertexts (per-precinct tallies): (1) every participant's ``DecryptionShareVerifier``
    checks its column of items, (2) one ``combine_shares_batch`` over the verdicts, (3) one ``DiscreteLogSolver.solve`` over [lo, hi) -
    or one lookup per element in `table` - over all decrypted elements.
    ciphertexts: m x 64 bytes (or a list of 64-byte ciphertexts); verifiers: [(participant index, DecryptionShareVerifier)], in the
    order in which shares are preferred; items: one bytes object of m items per verifier.
    Returns (values, combined, used, status): values[c] is the plaintext of ciphertext c, or None where fewer than `threshold` shares
    verified or the plaintext is outside the range / the table; status: the k x m verdicts."""
    if not isinstance(ciphertexts, (bytes, bytearray)):
        ciphertexts = b"".join(ciphertexts)
    verifiers, items = list(verifiers), list(items)
    if len(verifiers) != len(items):
        raise ValueError("one column of items per verifier")
    if (solver is None) == (table is None):
        raise ValueError("exactly one of solver and table is needed")
    m = len(ciphertexts) // 64
    status = []
    for (_, ver), column in zip(verifiers, items):
        if len(column) != 128 * m:
            raise ValueError("every column needs one 128-byte item per ciphertext")
        status += ver.verify_batch(column)
    _, plain, combined, used = combine_shares_batch(group, shares, threshold, bytes(ciphertexts), [i for i, _ in verifiers],
                                                    b"".join(items), status)
    elements = [plain[32 * c : 32 * c + 32] for c in range(m)]
    values = solver.solve(elements, lo, hi) if solver is not None else [table.get(e) for e in elements]
    return [v if ok else None for v, ok in zip(values, combined)], combined, used, status
