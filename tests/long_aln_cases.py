"""Pairs whose traceback has 32,768 columns or more (the statistics word once held 15 bits of length), seeded and built in code, with
their reference records.  Each case names the smallest shape that reaches its event; tests/test_long_aln.py asserts every precondition
from the reference (oracle_py.align_pair + traceback_lean), nothing is assumed.

  z-*   --gap-extend 0: a gap of any length costs its opening only, so a 200-residue query reaches 32,768 columns against one long target
        (A.B against A.J.B, J junk) at the cost of a 200 x 33 k box.
  tie   one residue pair x / y between two matching stretches that scores below two gap openings: the walk meets a cell with H == F == E.
  nat   default gap costs: only residues reach the length, a 32,768 x 32,768 box (about 15 s per pair on the CPU): their records come from
        the fixture tests/golden/long_aln.json (tests/golden/make_long_aln.py), their sequences from the seeds.
"""
import functools
import hashlib
import json
import os

import numpy as np

import util

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_aln.json")
FIELDS = ("score", "score_rev", "corrected", "qstart", "qend", "tstart", "tend", "aln_len", "idents", "pass_evalue", "accepted", "gap_opens")
Z_OPTS = "--gap-extend 0"
TIE_OPTS = "--gap-open 6 --gap-extend 1"
TIEZ_OPTS = "--gap-open 6 --gap-extend 0"
NAT_OPTS = ""
LIMIT15 = 1 << 15          # the first alignment length 15 bits do not hold
LIMIT16 = 1 << 16


def _rnd(rng, n):
    return rng.integers(0, 20, n, dtype=np.uint8), rng.integers(0, 20, n, dtype=np.uint8)


def _cat(*parts):
    return np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts])


def sha(seq):
    return hashlib.sha256(np.ascontiguousarray(seq[0], np.uint8).tobytes() + np.ascontiguousarray(seq[1], np.uint8).tobytes()).hexdigest()


def z_pair(seed, la, lb, lj):
    """q = A.B, t = A.J.B: with free extension the optimal path is A, one gap over J, B: la + lj + lb columns"""
    rng = np.random.default_rng(seed)
    a, b, j = _rnd(rng, la), _rnd(rng, lb), _rnd(rng, lj)
    return _cat(a, b), _cat(a, j, b)


def z_wide_pair(seed):
    """q = A.J1.B (2,100), t = A.J2.B (65,535), junk on both sides: the path wanders through it in hundreds of gaps of both directions"""
    rng = np.random.default_rng(seed)
    a, b = _rnd(rng, 100), _rnd(rng, 100)
    return _cat(a, _rnd(rng, 1900), b), _cat(a, _rnd(rng, 65335), b)


def tie_letters(p):
    """(x, y): residues (3Di, AA) whose substitution score is below two gap openings of 6, the most negative the matrices have"""
    S3 = np.array(p.S3[:], np.int32).reshape(21, 21)[:20, :20]
    SA = np.array(p.SA[:], np.int32).reshape(21, 21)[:20, :20]
    i3, ia = np.unravel_index(np.argmin(S3), S3.shape), np.unravel_index(np.argmin(SA), SA.shape)
    return (int(i3[0]), int(ia[0])), (int(i3[1]), int(ia[1])), int(S3[i3] + SA[ia])


def tie_pair(seed, p, la, lb, lj=0):
    """q = A.x.B (.C), t = A.y.B (.J.C): at the cell behind x / y the two single-residue gaps, in either order, beat the substitution"""
    rng = np.random.default_rng(seed)
    x, y, _ = tie_letters(p)
    one = lambda c: (np.array([c[0]], np.uint8), np.array([c[1]], np.uint8))
    a, b = _rnd(rng, la), _rnd(rng, lb)
    if not lj:
        return _cat(a, one(x), b), _cat(a, one(y), b)
    c, j = _rnd(rng, 100), _rnd(rng, lj)
    return _cat(a, one(x), b, c), _cat(a, one(y), b, j, c)


def nat_identical(seed, n):
    a = _rnd(np.random.default_rng(seed), n)
    return a, (a[0].copy(), a[1].copy())


def nat_mutated(seed, n=33000, sub3=0.12, suba=0.28, n_indel=130):
    """a copy with substitutions in both tracks and short insertions / deletions"""
    rng = np.random.default_rng(seed)
    a = _rnd(rng, n)
    b3, ba = a[0].copy(), a[1].copy()
    m = rng.random(n) < sub3; b3[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
    m = rng.random(n) < suba; ba[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
    for pos in sorted(rng.integers(50, n - 50, n_indel).tolist(), reverse=True):
        w = int(rng.integers(1, 4))
        if rng.random() < 0.5:
            b3 = np.delete(b3, slice(pos, pos + w)); ba = np.delete(ba, slice(pos, pos + w))
        else:
            ins = _rnd(rng, w + 1)
            b3 = np.insert(b3, pos, ins[0]); ba = np.insert(ba, pos, ins[1])
    return a, (b3, ba)


# name -> (options, builder of (q, t)); every case is checked in both orders
Z_CASES = {
    "z-walk-32767": (Z_OPTS, lambda p: z_pair(1, 100, 100, LIMIT15 - 1 - 200)),
    "z-walk-32768": (Z_OPTS, lambda p: z_pair(1, 100, 100, LIMIT15 - 200)),
    "z-long-32767": (Z_OPTS, lambda p: z_pair(2, 1100, 1100, LIMIT15 - 1 - 2200)),
    "z-long-32768": (Z_OPTS, lambda p: z_pair(2, 1100, 1100, LIMIT15 - 2200)),
    "z-wide": (Z_OPTS, lambda p: z_wide_pair(9)),
    "tie-small": (TIE_OPTS, lambda p: tie_pair(3, p, 120, 90)),
    "tie-z": (TIEZ_OPTS, lambda p: tie_pair(4, p, 100, 100, LIMIT15 - 301)),
}
NAT_CASES = {
    "nat-32767": dict(kind="identical", seed=11, n=LIMIT15 - 1),
    "nat-32768": dict(kind="identical", seed=12, n=LIMIT15),
    "nat-mutated": dict(kind="mutated", seed=13, n=33000),
}
NAT_SEQ_IDS = (0.6, 0.8)        # --min-seq-id of the nat runs: the mutated pair's reference identity lies strictly between them
# --min-seq-id of the runs of each option group: every case of the group is accepted under the first and rejected under the second
# (200 / 32,768 = 0.006 .. 2,200 / 32,767 = 0.067 in the z groups; 210 / 212 in tie-small).  tests/test_long_aln.py asserts it.
GROUP_SEQ_IDS = {Z_OPTS: (0.004, 0.1), TIEZ_OPTS: (0.004, 0.1), TIE_OPTS: (0.5, 0.995)}


def seq_ids_of(name):
    return GROUP_SEQ_IDS[Z_CASES[name][0]]


def nat_sequences(name):
    c = NAT_CASES[name]
    return nat_identical(c["seed"], c["n"]) if c["kind"] == "identical" else nat_mutated(c["seed"], c["n"])


def params(O, opts):
    """-c 0 and traceback statistics for every pair: the identity gate is applied by the tests, per threshold"""
    p = util.oracle_params(O, ("-c 0 " + opts).strip())
    p.want_tb = 1
    return p


def reference(O, p, q, t):
    """the oracle's record of the pair (q, t) and its walk's tie mark, for both orders: [(record dict, tie), (record dict, tie)]"""
    odb = O.OracleDb(s3=[q[0], t[0]], sa=[q[1], t[1]])
    out = []
    for a, b in ((0, 1), (1, 0)):
        r = O.align_pair(odb, p, a, b, O.min_score(odb, p, a))
        rec = {f: int(r[f]) for f in FIELDS}
        assert rec["pass_evalue"] == 1 and rec["accepted"] == 1, rec
        st = O.traceback_lean(odb, p, a, b, rec["qstart"], rec["qend"], rec["tstart"], rec["tend"])
        assert st[:3] == (rec["aln_len"], rec["idents"], rec["gap_opens"])
        out.append((rec, st[3]))
    return out


@functools.lru_cache(maxsize=None)
def z_case(name):
    """dict(opts, q, t, ref) of a z- or tie case; the reference is computed once per session (0.1 to 3 s)"""
    from oracle import oracle_py as O
    opts, build = Z_CASES[name]
    p = params(O, opts)
    q, t = build(p)
    return dict(name=name, opts=opts, q=q, t=t, ref=reference(O, p, q, t))


@functools.lru_cache(maxsize=None)
def nat_case(name):
    """the same for a nat case, the reference read from the fixture (its input hashes are checked against the seeds here)"""
    fx = json.load(open(FIXTURE))["cases"][name]
    q, t = nat_sequences(name)
    assert (sha(q), sha(t)) == (fx["sha256_q"], fx["sha256_t"]), "the fixture was made from other sequences than the seeds give"
    return dict(name=name, opts=NAT_OPTS, q=q, t=t, ref=[(fx["records"][k], fx["tie"][k]) for k in (0, 1)])


def seq_id(rec):
    """identities / length as the gate computes it (float32)"""
    return np.float32(rec["idents"]) / np.float32(rec["aln_len"])
