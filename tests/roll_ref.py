"""Pure-Python model of the voter-roll rule (include/eg_hip.h, "voter roll"): a dict from voter to the best (word, seq).  Every expected
value of tests/test_roll_cpu.py and tests/test_gpu_roll.py comes from here; nothing is derived from the code under test."""
ST_SUPERSEDED = 16
ROLL_FIRST, ROLL_LAST = 1, 2
SUPERSEDED, OFF_ROLL, NOT_CAST = 1, 2, 3
SEQ_NONE = (1 << 64) - 1
GROUP_NONE = 0xFFFFFFFF
KEYS_MAX = 1 << 31
SEQ_END = (1 << 63) - 1          # seq_base + n may reach it: the largest sequence number is 2^63 - 2


def word(seq: int, policy: int) -> int:
    assert 0 <= seq <= SEQ_END - 1 and policy in (ROLL_FIRST, ROLL_LAST)
    return seq + 1 if policy == ROLL_LAST else SEQ_END - seq


def seq(w: int, policy: int) -> int:
    assert 1 <= w <= SEQ_END and policy in (ROLL_FIRST, ROLL_LAST)
    return w - 1 if policy == ROLL_LAST else SEQ_END - w


def status_word(detail: int) -> int:
    return ST_SUPERSEDED | detail << 8


class Roll:
    """best[v] = (word, seq) of the counted ballot of voter v; voters without one are absent"""

    def __init__(self, n_keys: int, policy: int, words=None):
        self.n_keys, self.policy, self.best = n_keys, policy, {}
        for v, w in enumerate(words or []):
            if w:
                self.best[v] = (w, seq(w, policy))

    def words(self):
        return [self.best[v][0] if v in self.best else 0 for v in range(self.n_keys)]

    def _judge(self, key_index, seq_base, status_in, roster_groups, roster_weights, cast_rule):
        n = len(key_index)
        by, out, groups, weights, found = [SEQ_NONE] * n, [0] * n, [GROUP_NONE] * n, [0] * n, [0, 0, 0]
        for b in range(n):
            st = status_in[b] if status_in is not None else 0
            out[b] = st
            if st != 0:
                continue
            v = key_index[b]
            if v >= self.n_keys:
                out[b] = status_word(OFF_ROLL)
                found[2] += 1
                continue
            if v not in self.best:
                assert not cast_rule
                out[b] = status_word(NOT_CAST)
                found[1] += 1
                continue
            w, s = self.best[v]
            if w == word(seq_base + b, self.policy):
                groups[b] = roster_groups[v] if roster_groups is not None else GROUP_NONE
                weights[b] = roster_weights[v] if roster_weights is not None else 0
            else:
                out[b], by[b] = status_word(SUPERSEDED), s
                found[0] += 1
        return {"superseded_by": by, "status_out": out, "groups_out": groups if roster_groups is not None else None,
                "weights_out": weights if roster_weights is not None else None, "found": found}

    def cast(self, key_index, seq_base=0, status_in=None, roster_groups=None, roster_weights=None):
        """the new best of every voter, then the verdicts against it; displaced = (old seq, new seq) in the order of the winning ballots"""
        old = dict(self.best)
        for b, v in enumerate(key_index):
            if (status_in is None or status_in[b] == 0) and v < self.n_keys:
                s = seq_base + b
                cand = (word(s, self.policy), s)
                if v not in self.best or cand[0] > self.best[v][0]:
                    self.best[v] = cand
        res = self._judge(key_index, seq_base, status_in, roster_groups, roster_weights, True)
        moved = sorted((new[1], old[v][1]) for v, new in self.best.items() if v in old and old[v] != new)
        res["displaced"] = [(o, s) for s, o in moved]                  # inside a batch the sequence order is the ballot order
        res["found"][1] = len(moved)
        return res

    def check(self, key_index, seq_base=0, status_in=None, roster_groups=None, roster_weights=None):
        return self._judge(key_index, seq_base, status_in, roster_groups, roster_weights, False)

    def kept(self, key_index, seq_base=0, status_in=None):
        res = self.check(key_index, seq_base, status_in)
        return [b for b in range(len(key_index)) if res["status_out"][b] == 0]


def merge(a, b):
    """rolls of slabs, ranks or GPUs: the element-wise maximum of the words"""
    return [max(x, y) for x, y in zip(a, b)]
