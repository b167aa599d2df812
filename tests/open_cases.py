"""Cases of the ballot-audit pass shared by tests/test_open_cpu.py and tests/test_gpu_open.py: oracle-made ballots with the openings read
off the oracle's own draw trace, bare ciphertexts with pinned randomness, and the list of forgeries.  Every expected value comes from
tests/open_ref.py."""
import open_ref as R

L = R.L
POISON = 0xEE


class Opened:
    """One ballot with its opening: values[t] integers, rands[t] 32 bytes."""

    def __init__(self, ballot: bytes, values, rands):
        self.ballot, self.values, self.rands = bytes(ballot), [int(v) for v in values], [bytes(r) for r in rands]

    def copy(self):
        return Opened(self.ballot, self.values, self.rands)


def _draws(o, seed: int, count: int):
    rng = o.rng_from_u64(seed)
    return [o.rng_fill64(rng) for _ in range(count)]


def oracle_choice(o, op, seed: int, chosen, rng_skip: int = 0):
    """(Opened, trace positions of the ct_r draws): the ballot the oracle makes from rng_from_u64(seed) after rng_skip draws, opened by
    the scalar at each position of the untouched stream, reduced from 64 bytes mod l."""
    rng = o.rng_from_u64(seed)
    for _ in range(rng_skip):
        o.rng_fill64(rng)
    with o.Script() as s:
        ballot = op.new_ballot(chosen, rng)
    pos = [rng_skip + j for j, t in enumerate(s.trace) if t[0] == "ct_r"]
    assert [t[2] for t in s.trace if t[0] == "ct_r"] == list(range(op.n_options))
    draws = _draws(o, seed, rng_skip + len(s.trace))
    return Opened(ballot, [int(bool(c)) for c in chosen], [o.sc_from_wide(draws[p]) for p in pos]), pos


def oracle_qv(o, op, seed: int, votes, rng_skip: int = 0):
    """The same for a quadratic-voting ballot: the vote ciphertexts' randomness is the draw with role value_r and scope k < n_options."""
    rng = o.rng_from_u64(seed)
    for _ in range(rng_skip):
        o.rng_fill64(rng)
    with o.Script() as s:
        ballot = op.new_ballot(votes, rng)
    pos = [rng_skip + j for j, t in enumerate(s.trace) if t[0] == "value_r" and t[1] < op.n_options]
    assert [t[1] for t in s.trace if t[0] == "value_r"] == list(range(op.n_options + 1))
    draws = _draws(o, seed, rng_skip + len(s.trace))
    return Opened(ballot, votes, [o.sc_from_wide(draws[p]) for p in pos]), pos


def bare_choice(o, pk: bytes, size: int, pairs):
    """A choice-layout ballot of len(pairs) bare ciphertexts (v, r) with r pinned through the oracle's Script, around poisoned proof bytes."""
    key = o.PublicKey(pk)
    body = b""
    for v, r in pairs:
        with o.Script({("ct_r", 0, 0): r}) as s:
            body += key.encrypt_u64(v, o.rng_from_u64(1))
        assert s.trace[0][0] == "ct_r"
    assert len(body) == 64 * len(pairs) <= size
    return Opened(body + bytes([POISON]) * (size - len(body)), [v for v, _ in pairs], [(r % L).to_bytes(32, "little") for _, r in pairs])


def _int(r: bytes) -> int:
    return int.from_bytes(r, "little")


def _set_r(c: Opened, t: int, value: int):
    c.rands[t] = (value % (1 << 256)).to_bytes(32, "little")


def forge_r_plus_1(c, t, slots):
    _set_r(c, t, (_int(c.rands[t]) + 1) % L)


def forge_v_plus_1(c, t, slots):
    c.values[t] = (c.values[t] + 1) % (1 << 64)


def forge_v_minus_1(c, t, slots):
    c.values[t] = (c.values[t] - 1) % (1 << 64)


def forge_r_plus_l(c, t, slots):
    _set_r(c, t, _int(c.rands[t]) + L)


def forge_r_all_ones(c, t, slots):
    _set_r(c, t, (1 << 256) - 1)


def forge_swap_slots(c, t, slots):
    u = (t + 1) % len(slots)
    c.rands[t], c.rands[u] = c.rands[u], c.rands[t]
    c.values[t], c.values[u] = c.values[u], c.values[t]


def forge_flip_wire_r(c, t, slots):
    b = bytearray(c.ballot)
    b[slots[t] + 5] ^= 0x10
    c.ballot = bytes(b)


def forge_flip_wire_b(c, t, slots):
    b = bytearray(c.ballot)
    b[slots[t] + 32 + 31] ^= 0x01
    c.ballot = bytes(b)


FORGERIES = [forge_r_plus_1, forge_v_plus_1, forge_v_minus_1, forge_r_plus_l, forge_r_all_ones, forge_swap_slots, forge_flip_wire_r,
             forge_flip_wire_b]


def forge_other_opening(c, other):
    """ballot c under the opening of another ballot"""
    c.values, c.rands = list(other.values), list(other.rands)


def flat(cases):
    """(ballots bytes, values list, rand bytes) of a pile as the entry points take them"""
    return (b"".join(c.ballot for c in cases), [v for c in cases for v in c.values], b"".join(r for c in cases for r in c.rands))


def model(group, cases, slots, status_in=None):
    return R.check_batch(group, [c.ballot for c in cases], slots, [c.values for c in cases], [c.rands for c in cases], status_in)


def write_case(path, key: bytes, stride: int, slots, cases, status_in=None, alias=False, poison_others=True):
    """The file tests/hostcheck/opencheck.cpp reads.  Ballots that do not participate get poisoned ballot and opening bytes."""
    assert all(off % 32 == 0 for off in slots)
    lines = [f"{key.hex()} {len(cases)} {len(slots)} {stride} {int(status_in is not None)} {int(alias)}", " ".join(str(off // 32) for off in slots)]
    for b, c in enumerate(cases):
        st = 0 if status_in is None else status_in[b]
        ballot, values, rands = c.ballot, c.values, c.rands
        if st and poison_others:
            ballot, values, rands = bytes([POISON]) * stride, [0xEEEEEEEEEEEEEEEE] * len(slots), [bytes([POISON]) * 32] * len(slots)
        assert len(ballot) == stride
        lines.append(" ".join([str(st), ballot.hex()] + [str(v) for v in values] + [r.hex() for r in rands]))
    path.write_text("\n".join(lines) + "\n")
    return path
