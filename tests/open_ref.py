"""The rule of the ballot-audit pass (include/eg_hip.h, "ballot audits") in plain Python: an opened ballot re-encrypted and compared.
The group arithmetic is handed in as two functions, so the same rule runs over the oracle's primitives (`oracle_group`) and over
tests/pyref's group (`pyref_group`), which shares no code with the oracle."""
L = 2**252 + 27742317777372353535851937790883648493
ST_BAD_OPENING = 17
OPEN_BAD_SCALAR, OPEN_R, OPEN_B = 1, 2, 3
ITEMS_MAX = 1 << 31


def status_word(slot: int, check: int) -> int:
    return ST_BAD_OPENING | ((slot * 4 + check) << 8)


def detail(word: int):
    """(slot, check) of a status word of kind ST_BAD_OPENING."""
    assert word & 0xFF == ST_BAD_OPENING
    return (word >> 8) >> 2, (word >> 8) & 3


class Group:
    """encrypt(v, r) -> (R, B) bytes for integers 0 <= v < 2^64 and 0 <= r < L."""

    def __init__(self, encrypt):
        self.encrypt = encrypt


def oracle_group(o, key: bytes) -> Group:
    g = o.point_mul_generator((1).to_bytes(32, "little"))

    def encrypt(v, r):
        rb = r.to_bytes(32, "little")
        big = o.point_multi_mul(v.to_bytes(32, "little") + rb, g + key)
        assert big is not None
        return o.point_mul_generator(rb), big

    return Group(encrypt)


def pyref_group(key: bytes) -> Group:
    from pyref import ristretto as rs

    k = rs.decode(key)
    assert k is not None

    def encrypt(v, r):
        return rs.encode(rs.mul_generator(r)), rs.encode(rs.add(rs.mul_generator(v), rs.mul(r, k)))

    return Group(encrypt)


def choice_slots(n_options: int):
    """Byte offset of the 64 wire bytes R || B of every slot in a packed choice ballot."""
    return [64 * t for t in range(n_options)]


def qv_slots(n_options: int, vote_size: int):
    return [vote_size * t for t in range(n_options)]


def check_slot(group: Group, wire: bytes, v: int, rand: bytes) -> int:
    """0, or the check that failed, for one ciphertext: `wire` = its 64 bytes, `rand` = the 32 bytes of r."""
    assert len(wire) == 64 and len(rand) == 32 and 0 <= v < 1 << 64
    r = int.from_bytes(rand, "little")
    if r >= L:
        return OPEN_BAD_SCALAR
    big_r, big_b = group.encrypt(v, r)
    if big_r != wire[:32]:
        return OPEN_R
    if big_b != wire[32:]:
        return OPEN_B
    return 0


def check_ballot(group: Group, ballot: bytes, slots, values, rands) -> int:
    """The status word of a participating ballot: the first failure in slot order wins."""
    for t, off in enumerate(slots):
        c = check_slot(group, ballot[off:off + 64], values[t], rands[t])
        if c:
            return status_word(t, c)
    return 0


def check_batch(group: Group, ballots, slots, values, rands, status_in=None):
    """(status_out, found) over a pile: ballots = list of packed ballots, values[b][t], rands[b][t]; a ballot whose status_in word is not
    0 keeps it and nothing of it is looked at."""
    out, found = [], [0, 0]
    for b, ballot in enumerate(ballots):
        if status_in is not None and status_in[b] != 0:
            out.append(status_in[b])
            continue
        found[0] += 1
        w = check_ballot(group, ballot, slots, values[b], rands[b])
        found[1] += w != 0
        out.append(w)
    return out, found


# ---- where the generators draw the encryption randomness, in 64-byte draws of the ballot's stream (open_host.hpp has the same) ----------
def choice_r_draws(rng_skip: int, chosen):
    """chosen[k] = option k is selected; option k draws r, x and - where it is not chosen - a simulated response."""
    out, at = [], rng_skip
    for c in chosen:
        out.append(at)
        at += 2 if c else 3
    return out


def qv_r_draws(rng_skip: int, n_options: int, rings):
    """rings = [(size, step)] of the vote range: a range proof draws n_rings + sum(sizes) scalars whatever its value."""
    d = len(rings) + sum(size for size, _ in rings)
    return [rng_skip + k * d for k in range(n_options)]
