"""The corpus that tests/pyref (the pure-Python verifier) judges, and the fixture of its verdicts (test infrastructure; built
deterministically from fixed seeds, by the oracle's provers on the CPU and by the HIP provers on the GPU, which are byte-equal).

Four corpora, each a list of families (one verifier's parameters) of named cases (packed bytes):

  sweep    valid items at the smallest shapes at which each mechanism changes, three a shape, each with its twins from ONE mutation
           function (`twins`): a flipped low bit in a response, a flipped bit in the common challenge, a scalar as itself plus l, an
           element as its negative field representative, two option ciphertexts swapped, and two of these at once at different items.
  edge     every family of edge_ballots.FAMILY_NAMES under the golden key: the valid edge items and their tampered twins, built as
           tests/test_gpu_edge_ballots.py builds them.
  forgery  forgery_cases: ALL of single5/golden; of every other family every k-th forgery (FORGERY_STRIDE), plus the first forgery of
           every numbered category and of every status kind the family reaches where the stride missed it, so that no family loses a
           category or a kind (`forgery_sample` asserts it); with the family's valid objects and zero-randomness bases.
  objects  ballot OBJECTS of another shape than the election's (serde's layout), the only inputs that reach the *_LEN status kinds.

The fixture, tests/golden/pyref_verdicts.json (written by tests/golden/make_pyref_verdicts.py), holds per family, in this module's
order of cases, pyref's status word of every case, the first 8 hex digits of the SHA-256 of every case's bytes (the lookup key), ONE
SHA-256 over all the cases' SHA-256 digests (`family_digest`: what binds every byte; per-case digests in full made a file no one
could review) and, per election, the SHA-256 of pyref's tally of the accepted cases.  Case names live here, not in the file.  pyref's verdicts are computed on a
pool of processes (`judge`); nothing of pyref is run on the GPU machine, where the fixture is the judge.

Counts: 4375 cases in 66 families -- sweep 40 families, 1010 cases (3 valid items and their 7 or 8 twins a shape); edge 10 families,
1233 cases; forgery 14 families, 2115 cases (1812 of the corpus's 3732 forgeries, FORGERY_STRIDE and FORGERY_COUNTS below, with 303
valid objects and bases); objects 2 families, 17 cases.  `python tests/golden/make_pyref_verdicts.py --counts` prints the cases
and the pyref seconds of every family.
"""
from __future__ import annotations

import functools
import hashlib
import json
import random
from dataclasses import dataclass, field
from math import isqrt
from pathlib import Path

import commit_equiv_ref as CE
import edge_ballots as E
import forgery_cases as F
import pyref_judge
from oracle import oracle as o

L = o.L
P = 2**255 - 19
FIXTURE = Path(__file__).resolve().parent / "golden" / "pyref_verdicts.json"
KEY_NAME = "golden"

# every k-th forgery of a family (single5/golden: all).  k = the smallest value that kept the family's sample at about 30 s of
# pyref time (one process) when this was written; what decides is the reduced sample's cost, so cheap families keep k = 1.
FORGERY_STRIDE = {
    ("single5", "golden"): 1, ("single9", "golden"): 4, ("multi20", "golden"): 11, ("qv4x12", "golden"): 5,
    ("zero", "golden"): 1, ("bool", "golden"): 1, ("range12", "golden"): 1, ("range15", "golden"): 1, ("range1000", "golden"): 3,
    ("share", "golden"): 1, ("sumsq2", "golden"): 1, ("commit_equiv", "golden"): 1, ("single5", F.OTHER_KEY): 1, ("zero", F.OTHER_KEY): 1,
}
# (forgeries judged, forgeries of the family): the sample with its category and kind fill-ins; tests/test_pyref_cpu.py asserts them
FORGERY_COUNTS = {
    ("single5", "golden"): (296, 296), ("single9", "golden"): (121, 484), ("multi20", "golden"): (78, 847), ("qv4x12", "golden"): (134, 668),
    ("zero", "golden"): (54, 54), ("bool", "golden"): (67, 67), ("range12", "golden"): (148, 148), ("range15", "golden"): (162, 162),
    ("range1000", "golden"): (129, 383), ("share", "golden"): (48, 48), ("sumsq2", "golden"): (135, 135), ("commit_equiv", "golden"): (90, 90),
    ("single5", F.OTHER_KEY): (296, 296), ("zero", F.OTHER_KEY): (54, 54),
}
assert set(FORGERY_STRIDE) == set(FORGERY_COUNTS) == set(F.FAMILIES)


@dataclass(frozen=True)
class Case:
    name: str
    blob: bytes
    valid: bool = False          # a valid item (the verdict must be 0)

    @property
    def sha(self) -> str:
        return hashlib.sha256(self.blob).hexdigest()


@dataclass
class Judged:
    """One family of one corpus: `fam` carries the oracle's verifier and the HIP verifier's parameters (forgery_cases.Family),
    `spec` what pyref needs to build its own."""
    corpus: str
    fam: F.Family
    cases: list = field(default_factory=list)
    recipe: dict = field(default_factory=dict)       # sweep: how the valid items are made (by either prover)

    @property
    def label(self) -> str:
        return self.fam.name if self.corpus in ("sweep", "objects") else f"{self.fam.name}/{self.fam.key_name}"

    @property
    def id(self) -> str:
        return f"{self.corpus}:{self.label}"

    @property
    def spec(self) -> tuple:
        f = self.fam
        if f.kind in ("single", "multi"):
            return (f.kind, f.key, f.n_options)
        if f.kind == "qv":
            return ("qv", f.key, f.n_options, f.credits)
        if f.kind in ("zero", "bool"):
            return (f.kind, f.key)
        if f.kind == "range":
            return ("range", f.key, f.credits)
        if f.kind == "share":
            x = f.extra
            return ("share", f.key, x["shares"], x["threshold"], x["index"], x["participant_key"])
        if f.kind == "sumsq":
            return ("sumsq", f.key, f.n_options, f.extra["label"])
        return ("commit_equiv", f.key, f.extra["h"], f.extra["label"])


# ------------------------------------------------------------------ pyref, on a pool of processes (tests/pyref_judge.py)
pyref_verifier = pyref_judge.verifier
judge = pyref_judge.judge


def pyref_tally(spec: tuple, blobs: list, words: list) -> str:
    return pyref_verifier(spec).tally(blobs, words).hex()


# ------------------------------------------------------------------ the mutation function
def _flip(item: bytes, byte: int, bit: int) -> bytes:
    b = bytearray(item)
    b[byte] ^= 1 << bit
    return bytes(b)


def ciphertext_slots(jf: Judged) -> list:
    """Item index of R of every option ciphertext (B follows), for the kinds that have options."""
    f = jf.fam
    if f.kind in ("single", "multi", "sumsq"):
        return [2 * i for i in range(f.n_options)]
    if f.kind == "qv":
        return [i * (f.oracle_params.vote_size // 32) for i in range(f.n_options)]
    return []


def twins(jf: Judged, blob: bytes, index: int) -> list:
    """(name, bytes) of the tampered twins of the valid item number `index` of its family.  Items are chosen by position in the
    layout, rotated by `index` so that the three items of a shape touch different ones."""
    layout = jf.fam.layout
    it = F.items(blob)
    scalars = [i for i, k in enumerate(layout) if k == "S"]
    points = [i for i, k in enumerate(layout) if k == "P"]
    challenge, responses = scalars[0], scalars[1:]       # in every layout the first scalar is a challenge, responses follow
    resp = responses[(7 * index + len(responses) // 2) % len(responses)]
    s_item = scalars[(5 * index + 1) % len(scalars)]
    p_item = points[(3 * index + 1) % len(points)]
    plus_l = (F.num(it[s_item]) + L).to_bytes(32, "little")
    neg_rep = (P - F.num(it[p_item])).to_bytes(32, "little")
    out = [
        ("response_bit0", F.put(blob, {resp: _flip(it[resp], 0, 0)})),
        ("challenge_bit", F.put(blob, {challenge: _flip(it[challenge], 5 + index, 3)})),
        ("scalar_plus_l", F.put(blob, {s_item: plus_l})),
        ("element_neg_rep", F.put(blob, {p_item: neg_rep})),
    ]
    slots = ciphertext_slots(jf)
    if len(slots) >= 2:
        a, b = slots[index % len(slots)], slots[(index + 1) % len(slots)]
        out.append(("swap_ciphertexts", F.put(blob, {a: it[b], a + 1: it[b + 1], b: it[a], b + 1: it[a + 1]})))
    last_s = scalars[-1]
    out.append(("two_challenge_bit_and_last_scalar_plus_l",
                F.put(blob, {challenge: _flip(it[challenge], 1, 1), last_s: (F.num(it[last_s]) + L).to_bytes(32, "little")})))
    if p_item < s_item:                                  # a later malformed scalar behind an earlier malformed element
        out.append(("two_element_neg_rep_and_scalar_plus_l", F.put(blob, {p_item: neg_rep, s_item: plus_l})))
    out.append(("two_response_bit0_and_challenge_bit", F.put(blob, {resp: _flip(it[resp], 0, 0), challenge: _flip(it[challenge], 9, 6)})))
    return [(n, b) for n, b in out if b != blob]


# ------------------------------------------------------------------ the shape sweep
SINGLE_OPTIONS = (1, 2, 7, 8, 9, 16, 32, 33, 40)         # 7 / 8: the fused-tail boundary; 32 / 33: the second mask word
RANGE_BOUNDS = (2, 3, 4, 5, 12, 15, 16, 17, 100, 1000, 65536, 10**6)
QV_SHAPES = {(1, 1): ([0], [1], [1]), (2, 4): ([0, 0], [2, 0], [1, 1]), (3, 9): ([0, 0, 0], [3, 0, 0], [1, 2, 2]),
             (5, 15): ([3, 0, 1, 0, 2], [0] * 5, [1, 1, 1, 2, 2]), (5, 20): ([4, 2, 0, 0, 0], [0] * 5, [2] * 5),
             (4, 100): ([10, 0, 0, 0], [0] * 4, [5] * 4), (3, 10000): ([100, 0, 0], [0] * 3, [57, 57, 58])}
SUMSQ_VALUES = {1: ([0], [3], [9]), 2: ([0, 0], [1, 2], [7, 7]), 5: ([1, 3, 3, 7, 5], [0] * 5, [2, 0, 9, 1, 4]),
                16: (list(range(16)), [0] * 16, [5] * 16)}
SHARE = {"shares": 3, "threshold": 2, "index": 1, "secret": 777}
COMMIT_H = 5                                             # blinding base [5]G
SWEEP_NAMES = tuple([f"single{n}" for n in SINGLE_OPTIONS] + ["multi1", "multi5", "multi3of16", "multi7of40"]
                    + [f"range{b}" for b in RANGE_BOUNDS] + [f"qv{n}x{c}" for n, c in QV_SHAPES]
                    + [f"sumsq{n}" for n in SUMSQ_VALUES] + ["zero", "bool", "share", "commit_equiv"])


def _seed(name: str) -> int:
    """The base seed of a sweep family: item i draws from ChaChaRng::seed_from_u64(seed + i)."""
    return 41000 + 16 * SWEEP_NAMES.index(name)


def _multi_flags(name: str) -> tuple:
    if name == "multi1":
        return ([0], [1], [1])
    if name == "multi5":
        return ([0] * 5, [1] * 5, [0, 1, 1, 0, 1])
    k, n = (3, 16) if name == "multi3of16" else (7, 40)
    rnd = random.Random(name)
    out = []
    for _ in range(3):
        chosen = set(rnd.sample(range(n), k))
        out.append([int(i in chosen) for i in range(n)])
    return tuple(out)


def _sweep_family(name: str) -> Judged:
    pk = E.key(KEY_NAME)
    k = o.PublicKey(pk)
    if name.startswith(("single", "multi")):
        single = name.startswith("single")
        if single:
            n = int(name[6:])
            flags = tuple([int(i == c) for i in range(n)] for c in (0, n // 2, n - 1))
        else:
            flags = _multi_flags(name)
            n = len(flags[0])
        fam = F.Family(name, "single" if single else "multi", KEY_NAME, pk, n_options=n, oracle_params=o.ChoiceParams(pk, n, single),
                       layout=F.choice_layout(n, single))
        return Judged("sweep", fam, recipe={"flags": flags})
    if name.startswith("range"):
        bound = int(name[5:])
        pr = o.PreparedRange(bound)
        fam = F.Family(name, "range", KEY_NAME, pk, credits=bound, oracle_params=k, extra={"range": pr}, layout=F.range_layout(bound))
        return Judged("sweep", fam, recipe={"values": (0, 1, bound - 1)})
    if name.startswith("qv"):
        n, credits = (int(x) for x in name[2:].split("x"))
        fam = F.Family(name, "qv", KEY_NAME, pk, n_options=n, credits=credits, oracle_params=o.QvParams(pk, n, credits),
                       layout=F.qv_layout(n, credits))
        votes = QV_SHAPES[(n, credits)]
        assert all(sum(v * v for v in vs) <= credits and max(vs) <= isqrt(credits) for vs in votes)
        return Judged("sweep", fam, recipe={"votes": votes})
    if name.startswith("sumsq"):
        n = int(name[5:])
        fam = F.Family(name, "sumsq", KEY_NAME, pk, n_options=n, oracle_params=k, extra={"label": F.LABEL},
                       layout="P" * (2 * n + 2) + "S" * (2 * n + 2))
        return Judged("sweep", fam, recipe={"values": SUMSQ_VALUES[n]})
    if name == "zero":
        return Judged("sweep", F.Family(name, "zero", KEY_NAME, pk, oracle_params=k, layout="PPSS"), recipe={"n": 3})
    if name == "bool":
        return Judged("sweep", F.Family(name, "bool", KEY_NAME, pk, oracle_params=k, layout="PPSSS"), recipe={"values": (0, 1, 1)})
    if name == "share":
        x = {kk: SHARE[kk] for kk in ("shares", "threshold", "index")}
        x["participant_key"] = E.element(SHARE["secret"])
        fam = F.Family(name, "share", KEY_NAME, pk, extra=x, layout="PPSS")
        return Judged("sweep", fam, recipe={"randoms": tuple(E.element(98100 + i) for i in range(3))})
    assert name == "commit_equiv"
    fam = F.Family(name, "commit_equiv", KEY_NAME, pk, extra={"h": E.element(COMMIT_H), "label": F.LABEL},
                   layout="P" * CE.N_POINTS + "S" * (CE.N_ITEMS - CE.N_POINTS))
    return Judged("sweep", fam, recipe={"values": (0, 123, 2**40 + 1)})


def sweep_items_oracle(jf: Judged) -> list:
    """The three valid items of a sweep family from the oracle's provers."""
    f, r, seed = jf.fam, jf.recipe, _seed(jf.fam.name)
    p = f.oracle_params
    rng = lambda i: o.rng_from_u64(seed + i)             # noqa: E731
    if f.kind in ("single", "multi"):
        return [p.new_ballot(fl, rng(i)) for i, fl in enumerate(r["flags"])]
    if f.kind == "qv":
        return [p.new_ballot(v, rng(i)) for i, v in enumerate(r["votes"])]
    if f.kind == "range":
        return [p.encrypt_range(f.extra["range"], v, rng(i)) for i, v in enumerate(r["values"])]
    if f.kind == "zero":
        return [p.encrypt_zero(rng(i)) for i in range(r["n"])]
    if f.kind == "bool":
        return [p.encrypt_bool(bool(v), rng(i)) for i, v in enumerate(r["values"])]
    if f.kind == "sumsq":
        out = []
        for i, vals in enumerate(r["values"]):
            cts, proof = p.sumsq_snapshot(vals, rng(i))
            out.append(cts[64:] + cts[:64] + proof)      # value ciphertexts || sum ciphertext || proof
        return out
    if f.kind == "share":
        x = f.extra
        return [R_ + o.decryption_share_new(E.sc(SHARE["secret"]), R_, x["shares"], x["threshold"], f.key, x["index"], rng(i))
                for i, R_ in enumerate(r["randoms"])]
    return [CE.prove(f.key, f.extra["h"], f.extra["label"], v, rng(i))[0] for i, v in enumerate(r["values"])]


def sweep_items_gpu(jf: Judged, params) -> list:
    """The same three items from the HIP provers (`params` = jf.fam.gpu_params(eg, ctx))."""
    f, r, seed = jf.fam, jf.recipe, _seed(jf.fam.name)
    if f.kind in ("single", "multi"):
        raw = params.encrypt_selected(seed, 0, [sum(b << i for i, b in enumerate(fl)) for fl in r["flags"]])
    elif f.kind == "qv":
        raw = params.encrypt_votes(seed, 0, r["votes"])
    elif f.kind == "zero":
        raw = params.prove(seed, 0, r["n"])
    elif f.kind in ("range", "bool", "sumsq", "commit_equiv"):
        raw = params.prove(seed, 0, r["values"])
    else:
        raw, ok = params.prove(E.sc(SHARE["secret"]), seed, 0, b"".join(r["randoms"]))
        assert set(ok) == {1}
    return F._split(raw, f.size)


def _with_sweep_cases(jf: Judged, valid: list) -> Judged:
    assert len(valid) == 3 and all(len(v) == jf.fam.size for v in valid), jf.id
    cases = []
    for i, v in enumerate(valid):
        cases.append(Case(f"valid{i}", v, True))
        cases += [Case(f"valid{i}_{n}", b) for n, b in twins(jf, v, i)]
    jf.cases = cases
    return jf


@functools.lru_cache(None)
def sweep_family(name: str) -> Judged:
    jf = _sweep_family(name)
    return _with_sweep_cases(jf, sweep_items_oracle(jf))


def sweep_family_gpu(name: str, eg, ctx):
    """(Judged with its items made by the HIP prover, the params object, still open)."""
    jf = _sweep_family(name)
    params = jf.fam.gpu_params(eg, ctx)
    return _with_sweep_cases(jf, sweep_items_gpu(jf, params)), params


# ------------------------------------------------------------------ the edge corpus
def _edge_layout(fam) -> str:
    if fam.kind in ("single", "multi"):
        return F.choice_layout(fam.n_options, fam.kind == "single")
    if fam.kind == "qv":
        return F.qv_layout(fam.n_options, fam.credits)
    if fam.kind == "range":
        return F.range_layout(fam.credits)
    return {"zero": "PPSS", "bool": "PPSSS", "share": "PPSS"}[fam.kind]


@functools.lru_cache(None)
def edge_family(name: str) -> Judged:
    """The edge ballots with the twins of tests/test_gpu_edge_ballots.py (_with_twins): the challenge flipped, a random bit flipped."""
    e = E.family(name, KEY_NAME)
    fam = F.Family(e.name, e.kind, e.key_name, e.key, n_options=e.n_options, credits=e.credits, edges=e.edges, extra=e.extra,
                   oracle_params=e.oracle_params, layout=_edge_layout(e))
    cases, seen = [], set()
    for i, edge in enumerate(e.edges):
        for nm, blob, valid in ((edge.name, edge.ballot, True), (f"{edge.name}~challenge", E.tamper(edge.ballot, i, e.challenge_item), False),
                                (f"{edge.name}~random", E.tamper(edge.ballot, 1000 + i), False)):
            if blob not in seen:
                seen.add(blob)
                cases.append(Case(nm, blob, valid))
    return Judged("edge", fam, cases)


# ------------------------------------------------------------------ the forgery corpus
def forgery_sample(name: str, key_name: str) -> list:
    """Indices into forgery_cases.family(name, key_name).forgeries: every k-th, and the first of every category and status kind the
    stride missed."""
    fam = F.family(name, key_name)
    words = F.verdicts(name, key_name)
    k = FORGERY_STRIDE[(name, key_name)]
    picked = set(range(0, len(fam.forgeries), k))
    categories = {f.mutation for f in fam.forgeries}
    kinds = {w & 0xFF for w in words}
    for want, of in ((categories, lambda i: fam.forgeries[i].mutation), (kinds, lambda i: words[i] & 0xFF)):
        have = {of(i) for i in picked}
        for missing in sorted(want - have):
            picked.add(next(i for i in range(len(fam.forgeries)) if of(i) == missing))
    picked = sorted(picked)
    assert {fam.forgeries[i].mutation for i in picked} == categories, (name, key_name, "a category lost to the sampling")
    assert {words[i] & 0xFF for i in picked} == kinds, (name, key_name, "a status kind lost to the sampling")
    return picked


@functools.lru_cache(None)
def forgery_family(name: str, key_name: str) -> Judged:
    fam = F.family(name, key_name)
    cases = [Case(f"valid{i}", v, True) for i, v in enumerate(fam.valid)]
    cases += [Case(f"word_base{i}", v, True) for i, v in enumerate(fam.extra.get("word_bases", []))]
    cases += [Case(fam.forgeries[i].name, fam.forgeries[i].blob) for i in forgery_sample(name, key_name)]
    assert len({c.blob for c in cases}) == len(cases), (name, key_name)
    return Judged("forgery", fam, cases)


# ------------------------------------------------------------------ objects of another shape (the *_LEN kinds)
def _dumps(obj) -> bytes:
    return json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()


OBJECT_NAMES = ("single7", "qv5x20")


@functools.lru_cache(None)
def object_family(name: str) -> Judged:
    """Valid ballots of the sweep, unpacked into serde's layout and reshaped; a case's bytes are its JSON text (sorted keys)."""
    import copy

    from elastic_elgamal_amd import ingest, serde

    src = sweep_family(name)
    f = src.fam
    base = src.cases[0].blob
    cases = []
    if f.kind == "single":
        obj = serde.unpack_encrypted_choice(base, f.n_options, True)
        variants = {"as_is": lambda x: None,
                    "one_choice_fewer": lambda x: x["choices"].pop(),
                    "one_choice_more": lambda x: x["choices"].append(x["choices"][0]),
                    "two_responses_fewer": lambda x: [x["range_proof"]["ring_responses"].pop() for _ in range(2)],
                    "one_response_more": lambda x: x["range_proof"]["ring_responses"].append(x["range_proof"]["ring_responses"][0]),
                    "choice_fewer_and_bad_sum": lambda x: (x["choices"].pop(), x["sum_proof"].update(response=x["sum_proof"]["challenge"])),
                    "responses_fewer_and_bad_sum": lambda x: (x["range_proof"]["ring_responses"].pop(),
                                                              x["sum_proof"].update(response=x["sum_proof"]["challenge"]))}
    else:
        obj = ingest.unpack_qv_ballot(base, f.n_options, f.credits)
        rp = lambda x, i: (x["votes"][i] if i < f.n_options else x["credit"])["range_proof"]    # noqa: E731
        sq = lambda x: x["credit_equivalence_proof"]["ciphertext_responses"]                      # noqa: E731
        variants = {"as_is": lambda x: None,
                    "one_vote_fewer": lambda x: x["votes"].pop(),
                    "vote2_partial_more": lambda x: rp(x, 2)["partial_ciphertexts"].append(x["votes"][0]["ciphertext"]),
                    "vote4_response_fewer": lambda x: rp(x, 4)["ring_responses"].pop(),
                    "vote1_and_vote3_response_more": lambda x: [rp(x, i)["ring_responses"].append(rp(x, i)["common_challenge"]) for i in (3, 1)],
                    "credit_partial_fewer": lambda x: rp(x, f.n_options)["partial_ciphertexts"].pop(),
                    "credit_response_more": lambda x: rp(x, f.n_options)["ring_responses"].append(rp(x, 0)["common_challenge"]),
                    "sumsq_two_responses_fewer": lambda x: [sq(x).pop() for _ in range(2)],
                    "sumsq_response_more": lambda x: sq(x).append(sq(x)[0]),
                    "credit_partial_fewer_and_sumsq_fewer": lambda x: (rp(x, f.n_options)["partial_ciphertexts"].pop(), sq(x).pop())}
    for nm, change in variants.items():
        x = copy.deepcopy(obj)
        change(x)
        cases.append(Case(nm, _dumps(x), nm == "as_is"))
    return Judged("objects", f, cases)


def object_spec(jf: Judged) -> tuple:
    f = jf.fam
    return ("object", f.kind, f.key, f.n_options, f.credits)


def oracle_object_word(jf: Judged, text: bytes) -> int:
    """The oracle's verdict on an object of any shape (oracle/objects.c)."""
    from elastic_elgamal_amd.serde import b64url_decode as d

    x, f = json.loads(text), jf.fam
    ct = lambda c: (d(c["random_element"]), d(c["blinded_element"]))                              # noqa: E731
    if f.kind == "single":
        rp, sp = x["range_proof"], x["sum_proof"]
        return f.oracle_params.verify_object([ct(c) for c in x["choices"]], d(rp["common_challenge"]), [d(s) for s in rp["ring_responses"]],
                                             (d(sp["challenge"]), d(sp["response"])))
    blocks = [(ct(b["ciphertext"]), [ct(c) for c in b["range_proof"]["partial_ciphertexts"]], d(b["range_proof"]["common_challenge"]),
               [d(s) for s in b["range_proof"]["ring_responses"]]) for b in x["votes"] + [x["credit"]]]
    p = x["credit_equivalence_proof"]
    return f.oracle_params.verify_object(blocks, (d(p["challenge"]), [d(s) for s in p["ciphertext_responses"]], d(p["sum_response"])))


# ------------------------------------------------------------------ the whole corpus and its fixture
def all_ids() -> list:
    return ([("sweep", n, "") for n in SWEEP_NAMES] + [("edge", n, KEY_NAME) for n in E.FAMILY_NAMES]
            + [("forgery", n, k) for n, k in F.FAMILIES] + [("objects", n, "") for n in OBJECT_NAMES])


def judged(corpus: str, name: str, key_name: str = "") -> Judged:
    if corpus == "sweep":
        return sweep_family(name)
    if corpus == "edge":
        return edge_family(name)
    if corpus == "forgery":
        return forgery_family(name, key_name)
    return object_family(name)


def family_digest(cases: list) -> str:
    """SHA-256 over the SHA-256 digests of the cases' bytes, in the family's order: one number that binds every byte of a family."""
    return hashlib.sha256(b"".join(bytes.fromhex(c.sha) for c in cases)).hexdigest()


def fixture_entry(jf: Judged) -> dict:
    """What the fixture holds for one family, its cases in the module's order (their names are jf.cases[i].name): `n` their number,
    `digest` = family_digest, `sha8` the first 8 hex digits of every case's SHA-256 run together (the key an item is looked up by;
    unique within the family), `words` pyref's status words and, for elections, `tally_sha256` = the SHA-256 of pyref's tally of the accepted cases
    (n_options x (R || B), canonical encodings)."""
    blobs = [c.blob for c in jf.cases]
    words = judge(object_spec(jf) if jf.corpus == "objects" else jf.spec, blobs)
    prefixes = [c.sha[:8] for c in jf.cases]
    assert len(set(prefixes)) == len(prefixes), (jf.id, "two cases share a hash prefix: use another seed")
    entry = {"n": len(jf.cases), "digest": family_digest(jf.cases), "sha8": "".join(prefixes), "words": words}
    if jf.fam.tallies and jf.corpus != "objects":
        entry["tally_sha256"] = hashlib.sha256(bytes.fromhex(pyref_tally(jf.spec, blobs, words))).hexdigest()
    return entry


@functools.lru_cache(None)
def load_fixture() -> dict:
    return json.loads(FIXTURE.read_text())


def fixture_words(family_id: str) -> dict:
    """hash prefix -> status word of the committed fixture, for one family."""
    f = load_fixture()["families"][family_id]
    assert len(f["sha8"]) == 8 * f["n"] and len(f["words"]) == f["n"]
    return {f["sha8"][8 * i : 8 * i + 8]: w for i, w in enumerate(f["words"])}
