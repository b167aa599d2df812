"""Pure-Python model of ballot weeding (eg_*_weed*, include/eg_hip.h): a dict from key bytes to the earliest owner.

A ballot is a list of keys (64-byte strings).  Ballot b participates iff status[b] == 0 (status None: every ballot).  dup_of[b] is
DUP_NONE for a ballot that does not participate or shares no key, DUP_PRIOR if any key is on the board, otherwise the smallest b' < b
of a participating ballot that shares a key with b - whether or not b' is flagged itself."""
import random

DUP_NONE = 0xFFFFFFFF
DUP_PRIOR = 0xFFFFFFFE
ST_DUPLICATE = 14


def weed(ballot_keys, status=None, board=()):
    """-> (dup_of, status_out, appended keys of the participating, unflagged ballots in ballot and option order)"""
    n = len(ballot_keys)
    on_board = set(board)
    owner = {}
    for b, keys in enumerate(ballot_keys):
        if status is not None and status[b] != 0:
            continue
        for k in keys:
            owner.setdefault(k, b)
    dup_of, out, appended = [], [], []
    for b, keys in enumerate(ballot_keys):
        st = 0 if status is None else status[b]
        d = DUP_NONE
        if st == 0:
            if any(k in on_board for k in keys):
                d = DUP_PRIOR
            else:
                earlier = [owner[k] for k in keys if owner[k] < b]
                if earlier:
                    d = min(earlier)
            if d == DUP_NONE:
                appended += list(keys)
        dup_of.append(d)
        out.append(ST_DUPLICATE if d != DUP_NONE else st)
    assert len(dup_of) == n
    return dup_of, out, appended


def keys_of(ballots: bytes, stride: int, r_items):
    """the keys of packed ballots: 64 bytes from item r of every ballot, for r in r_items"""
    n = len(ballots) // stride
    return [[ballots[b * stride + 32 * r:b * stride + 32 * r + 64] for r in r_items] for b in range(n)]


def found(dup_of):
    return sum(d == DUP_PRIOR for d in dup_of), sum(d not in (DUP_NONE, DUP_PRIOR) for d in dup_of)


def planted(seed: int, n: int, n_keys: int, n_board: int = 0):
    """n ballots of n_keys random keys and a board of n_board, with every kind of copy planted (needs n >= 40, n_keys >= 2): whole
    ballots, one key at another option position, the chain A{x,y} B{y,z} C{z,w}, a key twice inside one ballot, copies of board
    entries, a copy of a copy.  -> (ballot keys, board keys)"""
    rng = random.Random(seed)
    key = lambda: bytes(rng.getrandbits(8) for _ in range(64))
    ballots = [[key() for _ in range(n_keys)] for _ in range(n)]
    board = [key() for _ in range(n_board)]
    ballots[7] = list(ballots[2])                                  # a whole copy
    ballots[n - 1] = list(ballots[0])                              # the last ballot copies the first
    ballots[11][n_keys - 1] = ballots[5][0]                        # one key, at another position
    ballots[21][1] = ballots[20][0]                                # the chain: 20 {x, y}, 21 {y', x}..
    ballots[22][0] = ballots[21][n_keys - 1] if n_keys > 2 else ballots[21][0]
    ballots[23][1] = ballots[22][n_keys - 1] if n_keys > 2 else ballots[22][1]
    ballots[30][1] = ballots[30][0]                                # twice inside one ballot: no duplicate
    ballots[33] = list(ballots[7])                                 # a copy of a copy: owned by 2
    if n_board:
        ballots[3][0] = board[0]
        ballots[35][n_keys - 1] = board[n_board - 1]
        ballots[36] = list(ballots[35])                            # on the board AND in the batch: the board wins
    return ballots, board
