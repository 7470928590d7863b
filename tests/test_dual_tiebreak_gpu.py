"""Both tie-break answers from one known-score DP (packed MODE 4 / 6, uc_sw_pk_impl.hpp key2) and what the gapped stage makes of them.

Raw passes (uc_engine_sw_pass2) on a pair list that holds every pair both ways round, over every packed class of tables 1 and 3: the second
answer of (q, t), roles swapped, is the oracle's answer for (t, q); the first answer and the one-row mark are what the pass reports
without the second outputs.  Pipeline: a database rich in tied mutual hits gives the oracle's records, with fewer known-score re-runs than
under the earlier sharing rule (UC_DUAL_TIEBREAK=0) and without a second start-pass round."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dual_util as D
import util
from test_sw_kernels import CAPS, TE_UNIQUE, Dp, _pmap, class_of

pytestmark = pytest.mark.gpu
PK_ROWS = 2048             # queries of the packed classes; longer ones take the int32 long-query kernel, which has no second answer
SMALL = 400                # pairs up to this size get the numpy DP (rows that hold an optimal cell)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.fixture(scope="module")
def both_ways(O):
    """the directed list: entries 2k = (q, t) and 2k + 1 = (t, q) of pair k; oracle answers of the forward pass and of the start pass.
    Start pass: entry i from the oracle's own end cell ("own"), and from its mirror's end cell transposed ("shared": the condition under
    which the gapped stage lets the two share one DP)"""
    import unicore_amd as U
    p = O.default_params()
    dp = Dp(p)
    s3, sa, pairs, kinds = D.tie_pairs(2025, D.sweep_lengths() + [2049], dp)
    q = np.array([x for a, b in pairs for x in (a, b)], np.uint32)
    t = np.array([x for a, b in pairs for x in (b, a)], np.uint32)
    n = len(q)
    mir = np.arange(n) ^ 1
    lens = np.array([len(x) for x in s3])
    fwd = np.array(_pmap(lambda i: O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p), range(n)), np.int64).reshape(n, 3)
    assert np.array_equal(fwd[:, 0], fwd[mir, 0])                      # symmetric matrices: one score for both directions
    assert fwd[:, 0].max() < D.SW_PK_OVF                                # inside the packed score range: raw passes answer every pair
    pos = np.nonzero(fwd[:, 0] > 0)[0]
    assert np.array_equal(np.sort(mir[pos]), pos)

    def start(i, qe, te):
        return O.sw(s3[q[i]][: qe + 1], sa[q[i]][: qe + 1], s3[t[i]][: te + 1], sa[t[i]][: te + 1], p, rev_q=1, rev_t=1)
    own_box = fwd[pos][:, 1:3]
    sh_box = fwd[mir[pos]][:, [2, 1]]
    st_own = np.array(_pmap(lambda k: start(pos[k], *own_box[k]), range(len(pos))), np.int64).reshape(len(pos), 3)
    st_sh = np.array(_pmap(lambda k: start(pos[k], *sh_box[k]), range(len(pos))), np.int64).reshape(len(pos), 3)
    assert np.array_equal(st_own[:, 0], fwd[pos, 0]) and np.array_equal(st_sh[:, 0], fwd[pos, 0])
    # numpy DP on the small entries: optimal rows of the forward DP and of the two start-pass DPs
    small = [k for k, i in enumerate(pos) if lens[q[i]] <= SMALL and lens[t[i]] <= SMALL]

    def rows(k):
        i = pos[k]
        H = dp.H(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]])
        assert D.first_answer(H) == tuple(fwd[i])                      # the numpy DP is the oracle's DP
        a = D.start_reference(dp, s3, sa, q[i], t[i], *own_box[k])
        b = D.start_reference(dp, s3, sa, q[i], t[i], *sh_box[k])
        assert a["st1"] == tuple(st_own[k]) and b["st1"] == tuple(st_sh[k])
        return D.optimal_rows_cols(H)[0], a["srows"], b["srows"], D.first_answer(H) != D.second_answer(H), a["st1"] != a["st2"]
    dps = dict(zip(small, _pmap(rows, small)))
    e = U.Engine("-c 0.8", verbosity=1)
    e.set_db(*util.flat(s3, sa))
    return dict(e=e, q=q, t=t, n=n, mir=mir, lens=lens, kinds=np.repeat(kinds, 2), fwd=fwd, pos=pos, own_box=own_box, sh_box=sh_box,
                st_own=st_own, st_sh=st_sh, dps=dps)


def _inputs_hold_ties(S):
    """a condition on the INPUTS, checked against the oracle / numpy DP alone: enough entries with more than one optimal row, and entries
    where the two tie-break orders pick different cells"""
    d = S["dps"].values()
    n4, n6o, n6s = sum(x[0] > 1 for x in d), sum(x[1] > 1 for x in d), sum(x[2] > 1 for x in d)
    assert n4 >= 50 and n6o >= 50 and n6s >= 50, (n4, n6o, n6s)
    assert sum(x[3] for x in d) >= 20 and sum(x[4] for x in d) >= 10, (sum(x[3] for x in d), sum(x[4] for x in d))


def _every_packed_class_ran(S, tab, cls, score):
    lens, q, pos = S["lens"], S["q"], S["pos"]
    assert np.array_equal(cls, [class_of(int(lens[x]), tab) for x in q[pos]])
    for c in range(len(CAPS[tab])):
        assert ((cls == c) & (score > 0)).any(), (tab, c)
    assert (cls == len(CAPS[tab])).any()                               # and the long-query kernel (no second answer)


@pytest.mark.parametrize("tab", [1, 3])
def test_mode4_second_answer_is_the_mirrors_end(both_ways, tab):
    S = both_ways
    _inputs_hold_ties(S)
    e, q, t, fwd, pos, mir = S["e"], S["q"], S["t"], S["fwd"], S["pos"], S["mir"]
    known = fwd[pos, 0].astype(np.int32)
    r = e.sw_pass(tab, 4, q[pos], t[pos], known=known, raw=True, second=True)
    r0 = e.sw_pass(tab, 4, q[pos], t[pos], known=known, raw=True)
    _every_packed_class_ran(S, tab, r["cls"], r["score"])
    for f in ("score", "qe", "te", "cls"):
        assert np.array_equal(r[f], r0[f]), f                          # the first answer does not depend on the second outputs
    assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1), fwd[pos])
    packed = S["lens"][q[pos]] <= PK_ROWS
    want = fwd[mir[pos]][:, [2, 1]]                                    # (t, q)'s (qend, tend), roles swapped
    got = np.stack([r["qe2"], r["te2"]], 1)
    bad = np.nonzero((got != want).any(1) & packed)[0]
    assert len(bad) == 0, (tab, len(bad), [(int(pos[k]), S["kinds"][pos[k]], got[k].tolist(), want[k].tolist()) for k in bad[:8]])
    assert (got[~packed] == -2).all() and (~packed).any()
    # with the library's re-run rules nothing changes here (no pair is flagged), and a second answer is still reported
    rr = e.sw_pass(tab, 4, q[pos], t[pos], known=known, second=True)
    assert np.array_equal(np.stack([rr["qe2"], rr["te2"]], 1), got)
    assert np.array_equal(np.stack([rr["score"], rr["qe"], rr["te"]], 1), fwd[pos])


@pytest.mark.parametrize("tab", [1, 3])
@pytest.mark.parametrize("box", ["own", "shared"])
def test_mode6_second_answer_is_the_mirrors_start(both_ways, tab, box):
    """entry i from box B and its mirror from B transposed are transposed DPs: "own" boxes of the entries 2k pair with "shared" boxes of 2k + 1
    and the other way round, so the second answer of (i, own) is the first of (mirror, shared) and vice versa"""
    S = both_ways
    _inputs_hold_ties(S)
    e, q, t, fwd, pos, mir = S["e"], S["q"], S["t"], S["fwd"], S["pos"], S["mir"]
    known = fwd[pos, 0].astype(np.int32)
    bx = S["own_box"] if box == "own" else S["sh_box"]
    st, st_other = (S["st_own"], S["st_sh"]) if box == "own" else (S["st_sh"], S["st_own"])
    ends = np.zeros((len(pos), 4), np.int32)
    ends[:, 1], ends[:, 3] = bx[:, 0], bx[:, 1]
    r = e.sw_pass(tab, 6, q[pos], t[pos], box=ends, known=known, raw=True, second=True)
    r0 = e.sw_pass(tab, 6, q[pos], t[pos], box=ends, known=known, raw=True)
    _every_packed_class_ran(S, tab, r["cls"], r["score"])
    for f in ("score", "qe", "te", "cls"):
        assert np.array_equal(r[f], r0[f]), f                          # first answer and one-row mark: as without the second outputs
    te = np.where(r["te"] >= 0, r["te"] & ~TE_UNIQUE, r["te"])
    assert np.array_equal(np.stack([r["score"], r["qe"], te], 1), st)
    packed = S["lens"][q[pos]] <= PK_ROWS
    uniq = (r["te"] >= 0) & ((r["te"] & TE_UNIQUE) != 0)
    col = 1 if box == "own" else 2
    for k, d in S["dps"].items():
        if packed[k]:
            assert uniq[k] == (d[col] == 1), (tab, box, int(pos[k]), d)
    assert not uniq[~packed].any()
    where = {int(i): k for k, i in enumerate(pos)}
    mk = np.array([where[int(mir[i])] for i in pos])
    want = st_other[mk][:, [2, 1]]                                     # the mirror's (qstart', tstart') from the transposed box, roles swapped
    got = np.stack([r["qe2"], r["te2"]], 1)
    bad = np.nonzero((got != want).any(1) & packed)[0]
    assert len(bad) == 0, (tab, box, len(bad), [(int(pos[k]), S["kinds"][pos[k]], got[k].tolist(), want[k].tolist()) for k in bad[:8]])
    assert (got[~packed] == -2).all() and (~packed).any()


def test_second_answer_only_where_there_is_one(both_ways):
    import unicore_amd as U
    S = both_ways
    e, q, t = S["e"], S["q"][:4], S["t"][:4]
    for tab, mode in ((1, 0), (1, 1), (0, 0)):
        with pytest.raises(U.UcError):
            e.sw_pass(tab, mode, q, t, second=True)


def _child(env_extra):
    env = dict(os.environ, UC_TIMING="1", **env_extra)
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, "tests", "dual_pipeline_run.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    passes = {}
    for section in r.stderr.split("== ")[1:]:
        name = section.splitlines()[0].strip()
        passes[name] = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"sw pass mode (\d+): (\d+) pairs", section)]
    return out, passes


def test_pipeline_tied_mutual_hits():
    """cluster_step and the staged API on a database of tied mutual hits: the oracle's records, clusters and algorithmic counters under both
    rules; with both answers from one DP there are strictly fewer known-score re-runs than under the earlier sharing rule, fewer MODE 4
    pairs, and ONE MODE 6 pass per call (every partner here is in a packed class) where the earlier rule needs a second round"""
    new, pn = _child({})
    old, po = _child({"UC_DUAL_TIEBREAK": "0"})
    print("\nnew rule:", json.dumps(new), pn, "\nearlier rule:", json.dumps(old), po)
    for o in (new, old):
        assert o["assign_equal"] and o["assign_equal_staged"] and o["hits_equal"] and o["bad_fields"] == [], o
        assert o["n_mutual_passers"] >= 100 and o["n_pass_evalue"] >= 200, o
    for k in ("cells_fwd", "cells_rev", "cells_start", "cells_tb", "n_gapped_alignments", "n_start_alignments"):
        assert new[k] == old[k], k                                      # what is computed, not how: unchanged
    assert new["n_pk_reruns"] < old["n_pk_reruns"], (new["n_pk_reruns"], old["n_pk_reruns"])
    assert new["n_sw_runs"] < old["n_sw_runs"] and new["cells_run"] < old["cells_run"] and new["sw_kernel_launches"] < old["sw_kernel_launches"]
    for name in ("cluster_step", "staged align"):
        m6n, m6o = [x for x in pn[name] if x[0] == 6], [x for x in po[name] if x[0] == 6]
        m4n, m4o = [x for x in pn[name] if x[0] == 4], [x for x in po[name] if x[0] == 4]
        assert len(m6n) == 1 and len(m6o) == 2, (name, m6n, m6o)        # the second round: gone / there (so the database does need it)
        assert m6n[0] == m6o[0]                                         # round 1 is the same pass
        assert len(m4n) == 1 and len(m4o) == 1 and 0 < m4n[0][1] < m4o[0][1], (name, m4n, m4o)
