"""Shared by tests/test_weighted_tally_cpu.py and tests/test_gpu_weighted_tally.py: what a weighted per-group tally must equal, by the
CPU oracle alone - oracle.point_multi_mul(weights as 32-byte little-endian scalars, the wire items behind one tally slot) is the
weighted sum of that slot - and the corner weights of a bit width."""
import random

GROUP_NONE = 0xFFFFFFFF
WIDTHS = (1, 2, 8, 31, 32, 33, 63, 64)
M64 = (1 << 64) - 1


def corner_weights(bits: int):
    """0, 1, 2, 3, 2^(W-1), 2^W - 1 and the two alternating patterns, cut to W bits"""
    mask = (1 << bits) - 1
    return [w & mask for w in (0, 1, 2, 3, 1 << (bits - 1), mask, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555)]


def random_weights(seed: int, n: int, bits: int):
    rng = random.Random(seed)
    return [rng.getrandbits(bits) for _ in range(n)]


def item_offsets(op):
    """byte offsets of the 2 n_options tally points (R, B per option) inside a packed ballot, as the oracle's own tally reads them"""
    step = getattr(op, "vote_size", 64)
    return [k * step + 32 * h for k in range(op.n_options) for h in (0, 1)]


def weighted_sum(oracle, weights, points):
    """canonical encoding of sum [w] P by the oracle; 32 zero bytes for the empty sum"""
    if not weights:
        return bytes(32)
    out = oracle.point_multi_mul(b"".join(int(w).to_bytes(32, "little") for w in weights), b"".join(points))
    assert out is not None
    return out


def expected(oracle, op, ballots: bytes, status, weights, groups, n_groups: int, weight_bits: int, only=None):
    """(tallies, weight_sums, counts, bad2) by the oracle.  A ballot counts if it is accepted, its group id is in range and its weight is
    below 2^weight_bits; bad2 = accepted, in-range ballots whose weight is not.  groups None: every ballot in group 0.  `only`: compute
    the tallies of just these groups (a dict g -> bytes instead of the concatenation)."""
    size, offs = op.ballot_size, item_offsets(op)
    members, bad2 = {}, 0
    for b, s in enumerate(status):
        g = 0 if groups is None else groups[b]
        if s != 0 or g == GROUP_NONE or g >= n_groups:
            continue
        if weights[b] >> weight_bits:
            bad2 += 1
            continue
        members.setdefault(g, []).append(b)
    counts = [len(members.get(g, ())) for g in range(n_groups)]
    sums = [sum(weights[b] for b in members.get(g, ())) for g in range(n_groups)]

    def one(g):
        bs = members.get(g, [])
        ws = [weights[b] for b in bs]
        return b"".join(weighted_sum(oracle, ws, [ballots[b * size + o:b * size + o + 32] for b in bs]) for o in offs)

    if only is not None:
        return {g: one(g) for g in only}, sums, counts, bad2
    return b"".join(one(g) for g in range(n_groups)), sums, counts, bad2
