"""Keccak-f[1600] after FIPS 202 section 3.2 (the five step mappings on a 5 x 5 array of lanes, round constants from the LFSR
of 3.2.5, rotation offsets from the walk of 3.2.2), and the sponge for SHA3-256 / SHAKE128 so that the permutation can be pinned
against hashlib."""

MASK = (1 << 64) - 1


def _rc_bit(t: int) -> int:
    """rc(t) of FIPS 202 algorithm 5."""
    if t % 255 == 0:
        return 1
    r = 1
    for _ in range(t % 255):
        r <<= 1
        if r & 0x100:
            r ^= 0x171
    return r & 1


ROUND_CONSTANTS = []
for _ir in range(24):
    _rc = 0
    for _j in range(7):
        _rc |= _rc_bit(_j + 7 * _ir) << ((1 << _j) - 1)
    ROUND_CONSTANTS.append(_rc)

# rho offsets: (x, y) walks (1, 0) -> (y, 2x + 3y), offset (t + 1)(t + 2) / 2 at step t
RHO = [[0] * 5 for _ in range(5)]
_x, _y = 1, 0
for _t in range(24):
    RHO[_x][_y] = ((_t + 1) * (_t + 2) // 2) % 64
    _x, _y = _y, (2 * _x + 3 * _y) % 5


def _rotl(v: int, n: int) -> int:
    return ((v << n) | (v >> (64 - n))) & MASK if n else v


def keccak_f1600(state: bytearray) -> None:
    """In place on 200 bytes; lane (x, y) is the little-endian word at byte 8 (x + 5 y)."""
    assert len(state) == 200
    a = [[int.from_bytes(state[8 * (x + 5 * y) : 8 * (x + 5 * y) + 8], "little") for y in range(5)] for x in range(5)]
    for rc in ROUND_CONSTANTS:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]                    # theta
        d = [c[(x - 1) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[0] * 5 for _ in range(5)]                                                            # rho and pi
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rotl(a[x][y], RHO[x][y])
        a = [[b[x][y] ^ (~b[(x + 1) % 5][y] & MASK & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]   # chi
        a[0][0] ^= rc                                                                              # iota
    for x in range(5):
        for y in range(5):
            state[8 * (x + 5 * y) : 8 * (x + 5 * y) + 8] = a[x][y].to_bytes(8, "little")


def _sponge(rate: int, suffix: int, msg: bytes, out_len: int) -> bytes:
    st = bytearray(200)
    padded = bytearray(msg) + bytes([suffix]) + bytes(-(len(msg) + 1) % rate)
    padded[-1] ^= 0x80
    for off in range(0, len(padded), rate):
        for i in range(rate):
            st[i] ^= padded[off + i]
        keccak_f1600(st)
    out = b""
    while len(out) < out_len:
        out += bytes(st[:rate])
        if len(out) < out_len:
            keccak_f1600(st)
    return out[:out_len]


def sha3_256(msg: bytes) -> bytes:
    return _sponge(136, 0x06, msg, 32)


def shake128(msg: bytes, out_len: int) -> bytes:
    return _sponge(168, 0x1F, msg, out_len)
