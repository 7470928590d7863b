"""Child process of tests/test_dual_tiebreak_gpu.py::test_pipeline_*: one database rich in tied mutual hits through Engine.cluster_step and
through the staged API, compared with the oracle; prints one JSON line (counters of the staged run).  Run with UC_TIMING=1: the per-pass lines
on stderr are the caller's view of which passes ran.  A process of its own because UC_DUAL_TIEBREAK is read once per process."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")

import dual_util as D      # noqa: E402
import util                # noqa: E402
from test_sw_kernels import Dp, _zero_partner      # noqa: E402


def tied_family_db(seed, dp, n_fam=24):
    """families of near-identical proteins whose pairwise DPs hold tied optima: copies that differ in a zero-scoring first / last residue pair
    (two optimal cells on one diagonal, forward pass / start pass), heads A rev(A) against rev(A) A (anti-ordered start cells) and tails
    likewise (anti-ordered end cells), and tandem repeats U^3, U^4, U^5"""
    rng = np.random.default_rng(seed)
    s3, sa = [], []

    def add(x):
        s3.append(np.ascontiguousarray(x[0], np.uint8)); sa.append(np.ascontiguousarray(x[1], np.uint8))

    for f in range(n_fam):
        n = int(rng.integers(10, 16))
        A = D._rnd(rng, n)
        rA = (A[0][::-1].copy(), A[1][::-1].copy())
        M = D._rnd(rng, int(rng.integers(90, 200)))
        X, Y = D._rnd(rng, 5), D._rnd(rng, 6)
        base = D._cat(A, rA, M)
        add(base)
        y3, ya = _zero_partner(dp.S3, dp.SA, base[0][-1], base[1][-1], rng)
        add((np.append(base[0][:-1], y3), np.append(base[1][:-1], ya)))                   # zero-end copy
        y3, ya = _zero_partner(dp.S3, dp.SA, base[0][0], base[1][0], rng)
        add((np.insert(base[0][1:], 0, y3), np.insert(base[1][1:], 0, ya)))               # zero-start copy
        add(D._cat(rA, A, M))                                                              # forked head
        add(D._cat(M, A, X, rA))                                                           # crossed tails ...
        add(D._cat(M, rA, Y, A))                                                           # ... against each other
        if f % 3 == 0:
            U = D._rnd(rng, int(rng.integers(24, 40)))
            for k in (3, 4, 5):
                add(D._cat(*([U] * k)))
    for L in (700, 9, 1):
        add(D._rnd(rng, L))
    return s3, sa


def main():
    import unicore_amd as U
    from oracle import oracle_py as O
    opts = "-c 0.5"
    p = util.oracle_params(O, opts)
    s3, sa = tied_family_db(99, Dp(p))
    off, c3, ca = util.flat(s3, sa)
    ref = O.cluster(O.OracleDb(s3=s3, sa=sa), p, threads=8)
    out = {}
    e = U.Engine(opts, verbosity=1)
    e.set_db(off, c3, ca)
    sys.stderr.write("== cluster_step\n")
    assign, _ = e.cluster_step()
    out["assign_equal"] = bool(np.array_equal(assign, ref["assign"]))
    e = U.Engine(opts, verbosity=1)
    e.set_db(off, c3, ca)
    e.prefilter()
    cnt, hits = e.hits()
    out["hits_equal"] = bool(np.array_equal(cnt, ref["hit_cnt"]))
    e.reset_stats()
    sys.stderr.write("== staged align\n")
    e.align()
    al = e.alns()
    ra = np.concatenate([ref["aln"][i, : cnt[i]] for i in range(len(cnt))])
    bad = [f for f in ("score", "score_rev", "corrected", "pass_evalue", "accepted", "aln_len", "idents") if not np.array_equal(al[f], ra[f])]
    pe = al["pass_evalue"] == 1
    bad += [f for f in ("qstart", "qend", "tstart", "tend") if not np.array_equal(al[f][pe], ra[f][pe])]
    out["bad_fields"] = bad
    out["n_pass_evalue"] = int(pe.sum())
    # mutual hits among the gate passers, and how many of those records hold a tie the two orders resolve differently is the oracle's business;
    # here: how many directed gate passers have their mirror in the list too
    q = np.repeat(np.arange(len(cnt)), cnt)[pe]
    t = hits["target"][pe]
    have = set(zip(q.tolist(), t.tolist()))
    out["n_mutual_passers"] = sum(1 for a, b in have if a != b and (b, a) in have)
    st = e.stats()
    for k in ("n_pk_reruns", "n_sw_runs", "cells_run", "sw_kernel_launches", "cells_fwd", "cells_rev", "cells_start", "cells_tb",
              "n_gapped_alignments", "n_start_alignments"):
        out[k] = int(st[k])
    out["assign_equal_staged"] = bool(np.array_equal(U.setcover(e.n, e.edges()), ref["assign"]))
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
