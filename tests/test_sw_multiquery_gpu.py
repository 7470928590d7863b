"""The packed gapped kernel with several tasks per workgroup (sw_pk_kernel<G, R, MODE, NW, K>, K > 1: the G = 16 classes of table 1 when a
class's lists are short): one pass at a time through Engine.sw_pass(table 1) on a generated 2-proteome database plus constructed sequences,
against the scalar oracle - exact integer comparisons.  The lists are built for what K > 1 adds: a workgroup whose tasks have 1, 2 and 3 pairs
(a one-pair slot next to another query's slots), a class whose task count is no multiple of K and a class of one task, two queries of one
class with different lengths (rows and masks from the slot's own task), a query with more pairs than a task holds (two tasks of one query
in one workgroup), neighbouring query ids in different classes.  That the multi-task kernel really served them is read from the engine
(stats: sw_multiquery_launches / sw_multiquery_tasks)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import util
from test_sw_kernels import TCAP, TE_UNIQUE, _mutate, _pmap, class_of

pytestmark = pytest.mark.gpu

MQ_CLASSES = range(1, 12)      # table 1: the G = 16 classes with R >= 4 (caps 64 .. 384) have a multi-task variant ...
MQ_NOT_IN_MODE4 = (3, 4, 6)    # ... but for MODE 4 at R = 8, 10, 14 (caps 128, 160, 224), whose variant would cost a wave per SIMD (sw_pk_class_queries)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _read_db(O, prefix):
    odb = O.OracleDb(prefix)
    n = int(odb.db.n)
    off = np.ctypeslib.as_array(odb.db.off, (n + 1,)).astype(np.int64)
    c3 = np.ctypeslib.as_array(odb.db.s3, (int(off[n]),)).copy()
    ca = np.ctypeslib.as_array(odb.db.sa, (int(off[n]),)).copy()
    return [c3[off[i]:off[i + 1]] for i in range(n)], [ca[off[i]:off[i + 1]] for i in range(n)]


@pytest.fixture(scope="module")
def cases(O, tmp_path_factory):
    import unicore_amd as U
    p = O.default_params()
    rng = np.random.default_rng(77)
    prefix = util.gen_synth_db(str(tmp_path_factory.mktemp("mq") / "db"), 2, 0x5EED0011, 600, 0.7)
    s3, sa = _read_db(O, prefix)
    n_gen = len(s3)
    gen_by_len = np.argsort([len(x) for x in s3])

    def add(x3, xa):
        s3.append(np.ascontiguousarray(x3, np.uint8)); sa.append(np.ascontiguousarray(xa, np.uint8))
        return len(s3) - 1

    def rnd(L):
        return rng.integers(0, 20, L, dtype=np.uint8), rng.integers(0, 20, L, dtype=np.uint8)

    pairs, label = [], {}

    def query(L, n_pairs, name, q=None):
        """a query of L residues with n_pairs targets: mutated copies, fragments of it, and unrelated generated sequences of all lengths"""
        q = add(*rnd(L)) if q is None else q
        q3, qa = s3[q], sa[q]
        label[name] = q
        for k in range(n_pairs):
            if k % 3 == 0:
                t = add(*_mutate(rng, q3, qa, 0.15))
            elif k % 3 == 1:
                a, w = int(rng.integers(0, max(1, L - 60))), int(rng.integers(30, 61))
                t = add(*_mutate(rng, q3[a:a + w], qa[a:a + w], 0.1, indels=False))
            else:
                t = int(gen_by_len[rng.integers(0, n_gen)])
            pairs.append((q, t))
        return q

    # class 160 (129 .. 160 rows): five tasks - no multiple of 2 or 4 - of 1, 2 and 3 pairs, queries at the cap, one below it and at 130
    query(130, 3, "q130"); query(159, 2, "q159")
    q160 = add(*rnd(160))
    q161 = add(*rnd(161))                 # the next query id, one residue longer: class 192, a class of exactly one task
    query(160, 1, "q160", q160); query(161, 2, "q161", q161)
    assert q161 == q160 + 1 and class_of(160, 1) + 1 == class_of(161, 1)
    query(145, 3, "q145"); query(150, 2, "q150")
    # class 128: queries with more pairs than a task holds (tcap = 64): 65 -> 2 tasks, 129 -> 3 tasks, beside lists of 1, 2, 3
    query(100, 65, "q100x65"); query(120, 129, "q120x129")
    query(97, 1, "q97"); query(128, 2, "q128"); query(110, 3, "q110")
    # one more G = 16 class (R = 20) with an odd task count
    query(300, 3, "q300"); query(320, 1, "q320"); query(289, 2, "q289")
    off, c3, ca = util.flat(s3, sa)
    e = U.Engine("-c 0.8", verbosity=1)
    e.set_db(off, c3, ca)
    q = np.array([x[0] for x in pairs], np.uint32)
    t = np.array([x[1] for x in pairs], np.uint32)
    n = len(q)
    fwd = np.array(_pmap(lambda i: O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p), range(n)), np.int64).reshape(n, 3)
    rev = np.array(_pmap(lambda i: O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p, rev_q=1)[0], range(n)), np.int64)
    pos = np.nonzero(fwd[:, 0] > 0)[0]

    def start(i):
        qe, te = fwd[i, 1], fwd[i, 2]
        return O.sw(s3[q[i]][: qe + 1], sa[q[i]][: qe + 1], s3[t[i]][: te + 1], sa[t[i]][: te + 1], p, rev_q=1, rev_t=1)
    st = np.array(_pmap(start, pos), np.int64).reshape(len(pos), 3)
    lens = np.array([len(x) for x in s3])
    return dict(e=e, q=q, t=t, n=n, fwd=fwd, rev=rev, pos=pos, st=st, lens=lens, label=label)


def _tasks(S, sel):
    """tasks per class of table 1 as the planner cuts the pair list q[sel]: per (class, query) ceil(pairs / tcap)"""
    per = {}
    qs, cnt = np.unique(S["q"][sel], return_counts=True)
    for x, c in zip(qs, cnt):
        k = class_of(int(S["lens"][x]), 1)
        per[k] = per.get(k, 0) + -(-int(c) // TCAP[1][k])
    return per


def test_lists_are_what_they_claim(cases):
    S = cases
    per = _tasks(S, np.arange(S["n"]))
    c160, c192, c128, c320 = class_of(160, 1), class_of(161, 1), class_of(128, 1), class_of(320, 1)
    assert per == {c160: 5, c192: 1, c128: 8, c320: 3}, per
    assert all(k in MQ_CLASSES for k in per)
    cnt = {int(x): int(c) for x, c in zip(*np.unique(S["q"], return_counts=True))}
    assert sorted(cnt[S["label"][k]] for k in ("q130", "q159", "q160", "q145", "q150")) == [1, 2, 2, 3, 3]
    assert cnt[S["label"]["q100x65"]] == TCAP[1][c128] + 1 and cnt[S["label"]["q120x129"]] == 2 * TCAP[1][c128] + 1
    assert S["label"]["q161"] == S["label"]["q160"] + 1       # neighbouring query ids
    # the two lengths of the 160 class have pairs with a score, so a wrong row offset or mask would change a MODE 6 answer
    for k in ("q130", "q159"):
        assert (S["fwd"][S["q"] == S["label"][k], 0] > 0).any(), k


def test_forward_and_reversed_query(cases):
    """MODE 0 (with the library's re-run rules) and MODE 1, and the packed kernel's own MODE 0 scores (raw)"""
    S = cases
    e, q, t = S["e"], S["q"], S["t"]
    r = e.sw_pass(1, 0, q, t)
    assert np.array_equal(r["cls"], [class_of(int(S["lens"][x]), 1) for x in q])
    assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1), S["fwd"])
    assert np.array_equal(e.sw_pass(1, 1, q, t)["score"], S["rev"])
    # the kernel's own answers (raw: one plan, no re-run): two passes over the list, each through the multi-task variant of all four classes
    e.reset_stats()
    assert np.array_equal(e.sw_pass(1, 0, q, t, raw=True)["score"], S["fwd"][:, 0])
    assert np.array_equal(e.sw_pass(1, 1, q, t, raw=True)["score"], S["rev"])
    st = e.stats()
    per = _tasks(S, np.arange(S["n"]))
    assert st["sw_multiquery_launches"] == 2 * len(per) and st["sw_multiquery_tasks"] == 2 * sum(per.values()), (st["sw_multiquery_launches"], st["sw_multiquery_tasks"], per)


def test_known_score_passes(cases):
    """MODE 4 and MODE 6, raw, with the second answer asked for: the oracle's ends on every pair (MODE 6: rows counted from each query's own end)"""
    S = cases
    e, q, t, fwd, pos, st = S["e"], S["q"], S["t"], S["fwd"], S["pos"], S["st"]
    known = fwd[pos, 0].astype(np.int32)
    ends = np.zeros((len(pos), 4), np.int32)
    ends[:, 1], ends[:, 3] = fwd[pos, 1], fwd[pos, 2]
    e.reset_stats()
    r = e.sw_pass(1, 4, q[pos], t[pos], known=known, raw=True, second=True)
    assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1), fwd[pos])
    r = e.sw_pass(1, 6, q[pos], t[pos], box=ends, known=known, raw=True, second=True)
    te = np.where(r["te"] >= 0, r["te"] & ~TE_UNIQUE, r["te"])
    assert np.array_equal(np.stack([r["score"], r["qe"], te], 1), st)
    per = _tasks(S, pos)
    per4 = {k: v for k, v in per.items() if k not in MQ_NOT_IN_MODE4}
    assert len(per4) >= 2 and len(per4) < len(per)
    stt = e.stats()
    assert stt["sw_multiquery_launches"] == len(per) + len(per4) and stt["sw_multiquery_tasks"] == sum(per.values()) + sum(per4.values())
    for k in ("q130", "q159", "q160", "q161"):
        assert (q[pos] == S["label"][k]).any(), k


def test_same_answers_with_one_task_per_workgroup(tmp_path):
    """the same random 4,000-pair list with UC_SW_TASK_QUERIES=1 (one task per workgroup everywhere) and with the default: every output array of
    modes 0, 1, 4 and 6 equal, the second answers of 4 / 6 included; the default run took the multi-task kernel, the other did not"""
    got = {}
    for name, env in (("one", {"UC_SW_TASK_QUERIES": "1"}), ("default", {})):
        envp = dict(os.environ, UC_ALLOW_SYNTHETIC="1", **env)
        envp.pop("UC_SW_TASK_SLOTS", None)
        if not env:
            envp.pop("UC_SW_TASK_QUERIES", None)
        out = str(tmp_path / (name + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(util.ROOT, "tests", "sw_multiquery_run.py"), str(tmp_path), out], env=envp,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:]
        got[name] = dict(np.load(out))
    a, b = got["one"], got["default"]
    assert set(a) == set(b)
    for k in a:
        if k != "multiquery":
            assert np.array_equal(a[k], b[k]), k
    assert a["multiquery"][0] == 0 and a["multiquery"][1] == 0
    assert b["multiquery"][0] >= 10 and b["multiquery"][1] >= 100, b["multiquery"]
    assert b["multiquery"][2] >= 500                                       # pairs with a score: the known-score passes ran on something
    assert (b["m6_qe2"] >= 0).sum() >= 100 and len(np.unique(b["m0_cls"])) >= 4
