"""Cases of the shuffle verifier shared by tests/test_shuffle_cpu.py and tests/test_gpu_shuffle.py: an honest shuffle of n rows and its
twins - the same statement and proof with one thing wrong (tampered), or a proof made by an otherwise honest prover on a false statement
(lying).  A twin is a dict(name, ins, outs, K, key, prefix, proof); what it must give is the model's verdict (tests/shuffle_ref.py, the
oracle backend judging), except where a test states the bits."""
import random

import shuffle_ref as m

PREFIX = b"election-7/mixer-1"
SEED = b"eg-shuffle test key"
NOT_A_POINT = b"\xff" * 32                 # s >= p: never decodes
SCALARS = {"zero": 0, "one": 1, "l-1": m.L - 1, "l": m.L, "max": (1 << 256) - 1}


def flip(b: bytes, at: int, bit: int = 1) -> bytes:
    a = bytearray(b)
    a[at] ^= bit
    return bytes(a)


def put(proof: bytes, n: int, section: str, k: int, value: bytes) -> bytes:
    """the proof with 32 bytes replaced: a head field (t1 .. s4) or row k of c, chat, that, shat, sprime"""
    head = ["t1", "t2", "t3", "t41", "t42", "s1", "s2", "s3", "s4"]
    at = 32 * head.index(section) if section in head else m.HEAD + (["c", "chat", "that", "shat", "sprime"].index(section) * n + k) * 32
    return proof[:at] + value + proof[at + 32:]


def get(proof: bytes, n: int, section: str, k: int = 0) -> bytes:
    head = ["t1", "t2", "t3", "t41", "t42", "s1", "s2", "s3", "s4"]
    at = 32 * head.index(section) if section in head else m.HEAD + (["c", "chat", "that", "shat", "sprime"].index(section) * n + k) * 32
    return proof[at:at + 32]


def base(case, K, key, prefix=PREFIX):
    return {"name": "honest", "ins": case["ins"], "outs": case["outs"], "K": K, "key": key, "prefix": prefix, "proof": case["proof"]}


def tampered(case, K, key, full=True):
    """one flipped bit in every section of the statement, key, prefix and proof; bad encodings and scalars.  full = False: the few
    that large sizes can afford (each is a whole run of the model)."""
    n = len(case["ins"])
    b = base(case, K, key)
    k = n // 2
    proof = case["proof"]
    out = []

    def twin(name, **kw):
        out.append(dict(b, name=name, **kw))

    twin("sprime_bit", proof=put(proof, n, "sprime", k, flip(get(proof, n, "sprime", k), 3)))
    twin("shat_is_l", proof=put(proof, n, "shat", n - 1, m.L.to_bytes(32, "little")))
    twin("c_not_a_point", proof=put(proof, n, "c", 0, NOT_A_POINT))
    if not full:
        return out
    for sec in ("t1", "t2", "t3", "t41", "t42", "s1", "s2", "s3", "s4"):
        twin(sec + "_bit", proof=put(proof, n, sec, 0, flip(get(proof, n, sec), 5, 2)))
    for sec in ("c", "chat", "that", "shat"):
        twin(sec + "_bit", proof=put(proof, n, sec, k, flip(get(proof, n, sec, k), 7, 8)))
    twin("in_R_bit", ins=case["ins"][:k] + [flip(case["ins"][k], 2)] + case["ins"][k + 1:])
    twin("in_B_bit", ins=case["ins"][:k] + [flip(case["ins"][k], 40)] + case["ins"][k + 1:])
    twin("out_R_bit", outs=case["outs"][:k] + [flip(case["outs"][k], 9)] + case["outs"][k + 1:])
    twin("out_B_bit", outs=case["outs"][:k] + [flip(case["outs"][k], 63, 16)] + case["outs"][k + 1:])
    twin("key_H0_bit", key=[flip(key[0], 11)] + list(key[1:]))
    twin("key_Hk_bit", key=list(key[:k + 1]) + [flip(key[k + 1], 1)] + list(key[k + 2:]))
    twin("K_bit", K=flip(K, 6))
    twin("prefix_bit", prefix=flip(PREFIX, 0))
    twin("prefix_empty", prefix=b"")
    twin("s4_is_max", proof=put(proof, n, "s4", 0, b"\xff" * 32))
    twin("sprime_is_l", proof=put(proof, n, "sprime", 0, m.L.to_bytes(32, "little")))
    twin("chat_last_not_a_point", proof=put(proof, n, "chat", n - 1, NOT_A_POINT))
    twin("chat_first_not_a_point", proof=put(proof, n, "chat", 0, NOT_A_POINT))
    twin("out_R_not_a_point", outs=case["outs"][:k] + [NOT_A_POINT + case["outs"][k][32:]] + case["outs"][k + 1:])
    twin("in_B_not_a_point", ins=[case["ins"][0][:32] + NOT_A_POINT] + case["ins"][1:])
    twin("K_not_a_point", K=NOT_A_POINT)
    twin("H0_not_a_point", key=[NOT_A_POINT] + list(key[1:]))
    twin("HN_not_a_point", key=list(key[:n]) + [NOT_A_POINT] + list(key[n + 1:]))
    twin("t1_not_canonical", proof=put(proof, n, "t1", 0, NOT_A_POINT))
    return out


def lying(be, case, K, key, seed, full=True):
    """an otherwise honest prover on a false statement; name -> twin.  that_flip: a wrong t^_k with the challenge that follows from it
    (only CHAIN and row k); other_message: one output re-encrypts another message (exactly T41); two_on_one_H: c commits two rows to one
    generator (T1 and / or T3); the rest: a proof made under another prefix, K or key seed."""
    n = len(case["ins"])
    b = base(case, K, key)
    ins, outs, src, rho = case["ins"], case["outs"], case["src"], case["rho"]
    k = n // 2
    out = []
    out.append(dict(b, name="that_flip", row=k, proof=m.prove(be, ins, outs, K, key, PREFIX, src, rho, random.Random(seed + 1), that_flip=k)))
    delta = be.mul_generator([5])[0]
    wrong = outs[:k] + [outs[k][:32] + be.point_add([outs[k][32:]], [delta])[0]] + outs[k + 1:]
    out.append(dict(b, name="other_message", outs=wrong, proof=m.prove(be, ins, wrong, K, key, PREFIX, src, rho, random.Random(seed + 2))))
    if not full:
        return out
    if n >= 2:
        pi = [0] * n
        for i in range(n):
            pi[src[i]] = i
        pi[src[0]] = pi[src[1]]
        out.append(dict(b, name="two_on_one_H", proof=m.prove(be, ins, outs, K, key, PREFIX, src, rho, random.Random(seed + 3), pi=pi)))
    out.append(dict(b, name="other_prefix", proof=m.prove(be, ins, outs, K, key, b"election-7/mixer-2", src, rho, random.Random(seed + 4))))
    K2 = be.mul_generator([12345])[0]
    out.append(dict(b, name="other_K", proof=m.prove(be, ins, outs, K2, key, PREFIX, src, rho, random.Random(seed + 5))))
    key2 = m.derive_key(be, SEED + b"2", n)
    out.append(dict(b, name="other_key_seed", proof=m.prove(be, ins, outs, K, key2, PREFIX, src, rho, random.Random(seed + 6))))
    return out


def judge(be, t):
    return m.verify(be, t["ins"], t["outs"], t["K"], t["key"], t["prefix"], t["proof"])
