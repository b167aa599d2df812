"""Shared by tests/test_group_tally_cpu.py and tests/test_gpu_group_tally.py: what a per-group tally must equal (the oracle's tally of
each group's subset), the piece / level arithmetic counted directly, and the production piece sizes read from the product's header."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
GROUP_NONE = 0xFFFFFFFF


def piece_sizes():
    """(S1, S2) as group_tally_host.hpp names them for the launch sites"""
    text = (CSRC / "group_tally_host.hpp").read_text()
    s1 = int(re.search(r"constexpr uint32_t S1 = (\d+);", text).group(1))
    s2 = int(re.search(r"constexpr uint32_t S2 = (\d+);", text).group(1))
    return s1, s2


def expected(op, ballots: bytes, status, groups, n_groups: int, only=None):
    """(tallies, counts) by the oracle: tallies[g] = op.tally of the accepted ballots with groups[b] == g (Ciphertext::zero() - zero
    bytes - for none).  `only`: compute just these groups (a dict g -> bytes is returned instead of the concatenation)."""
    size, width = op.ballot_size, 64 * op.n_options
    members = {}
    for b, (s, g) in enumerate(zip(status, groups)):
        if s == 0 and g != GROUP_NONE and g < n_groups:
            members.setdefault(g, []).append(b)
    counts = [len(members.get(g, ())) for g in range(n_groups)] if only is None else None

    def one(g):
        bs = members.get(g)
        if not bs:
            return bytes(width)
        return op.tally(b"".join(ballots[b * size:(b + 1) * size] for b in bs), [0] * len(bs))

    if only is not None:
        return {g: one(g) for g in only}, {g: len(members.get(g, ())) for g in only}
    return b"".join(one(g) for g in range(n_groups)), counts


def depth(n: int, s1: int, s2: int) -> int:
    """levels that n ballots need, in closed form: 1 for n <= S1, else 1 + ceil(log_S2(ceil(n / S1)))"""
    m, k = -(-n // s1), 0
    while s2 ** k < m:
        k += 1
    return 1 + k


def scan_reference(counts, s1: int, s2: int):
    """offsets, and per level (pieces, piece0, group of every piece), counted directly"""
    levels = depth(sum(counts), s1, s2)
    offsets, run = [], 0
    for c in counts:
        offsets.append(run)
        run += c
    out, cur = [], list(counts)
    for l in range(levels):
        s = s1 if l == 0 else s2
        pieces = [-(-c // s) for c in cur]
        piece0, run = [], 0
        for p in pieces:
            piece0.append(run)
            run += p
        buckets = [g for g, p in enumerate(pieces) for _ in range(p)]
        out.append((pieces, piece0, buckets))
        cur = pieces
    return levels, offsets, out


def count_vectors(s: int):
    """group-count vectors for piece size s (S1 = S2 = s): empty groups leading, trailing and consecutive; all in one group; every group
    of size 1; sizes s - 1, s, s + 1, s^2 - 1, s^2, s^2 + 1"""
    sizes = [s - 1, s, s + 1, s * s - 1, s * s, s * s + 1]
    return [
        [0, 0, 3, 0, 0, 1, 0],
        [0, 5],
        [5, 0, 0],
        [0],
        [17],
        [0, 0, 17, 0],
        [1] * 9,
        sizes,
        [0] + sizes + [0, 0],
        list(reversed(sizes)),
    ] + [[c] for c in sizes]
