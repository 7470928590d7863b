"""The accept gates of the gapped stage on the GPU at their exact thresholds (cases, option sets and references: tests/gate_cases.py; that
they are what they claim: tests/test_gate_cases.py).

len_gate_kernel, gate_kernel (both passes), finalize_kernel, tb_apply_kernel and tbm_resolve_kernel decide with a float quotient against a
float threshold, or with two integers.  Every option set runs Engine.align on hit lists given with set_hits (no prefilter) and compares every
record, field by field, with the scalar oracle AND with the closed form - the intended integers pushed through the spec's rule in
numpy.float32.  Each list holds every pair in both directions and is run twice: as one align() call, where a mirror (t, q) takes score, ends,
starts and traceback statistics from the DP of (q, t), and query by query, where every direction is computed alone.  The routes: packed
classes (default), --sw-kernel i32, queries of 2,060 residues (long-query kernel), scores past the packed range (int32 re-run).
"""
import numpy as np
import pytest

import gate_cases as G
import util

pytestmark = pytest.mark.gpu


def _engine_options(o, tmp_path):
    opts = (o.opts() + " " + o.extra).strip()
    if o.table:
        path = str(tmp_path / "thresholds.txt")
        np.savetxt(path, G.eval_table(o.table), fmt="%d")
        opts += " --single-step-clustering --min-score-table " + path
    return opts


def _runs(o, tmp_path):
    """[(records, edges, stats)] of the option set's list as one align() call and as one call per query"""
    import unicore_amd as U
    g = o.group()
    e = U.Engine(_engine_options(o, tmp_path), verbosity=1)
    e.set_db(*util.flat(g.s3, g.sa))
    hits = np.zeros(len(g.pairs), U.HIT_DTYPE)
    hits["target"] = g.t
    out = []
    for per_query in (False, True):
        e.set_hits(g.counts, hits)
        e.reset_stats()
        if per_query:
            for q in np.nonzero(g.counts)[0]:
                e.align(int(q), int(q) + 1)
        else:
            e.align()
        out.append((e.alns().copy(), e.edges().copy(), e.stats()))
    e.close()
    return out


def _check(o, al, edges, st, how):
    """every record against the oracle and the closed form, the first differences named; the edge list; the alignment counter"""
    g, ora, thr = o.group(), G.oracle_records(o), G.thresholds(o, o.group())
    assert len(al) == len(g.pairs)
    bad, let_through = [], 0
    for i, pr in enumerate(g.pairs):
        got = {f: int(al[f][i]) for f in G.FIELDS}
        if "-a" not in o.extra.split():          # the cluster path computes length and identities; the gap count belongs to -a and the search path
            if got["gap_opens"] != 0:
                bad.append("%s: gap count %d without -a" % (pr["label"], got["gap_opens"]))
            got["gap_opens"] = ora[i]["gap_opens"]
        got = G.normalised(got)
        exp = G.expected(o, pr, int(thr[pr["q"]]))
        let_through += G.length_gate_lets_through(o, pr["lq"], pr["lt"])
        for name, ref in (("oracle", ora[i]), ("closed form", G.normalised(exp) if exp is not None else None)):
            if ref is not None and got != ref:
                diff = {f: (got[f], ref[f]) for f in G.FIELDS if got[f] != ref[f]}
                bad.append("%s, query %d -> target %d, %s, %s: (engine, %s) %s" % (pr["label"], pr["q"], pr["t"], o.name, how, name, diff))
    assert not bad, "%d differences, the first:\n%s" % (len(bad), "\n".join(bad[:8]))
    want = sorted((pr["q"], pr["t"]) for pr, r in zip(g.pairs, ora) if r["accepted"])
    assert sorted(map(tuple, edges.tolist())) == want, (o.name, how)
    assert st["n_gapped_alignments"] == let_through and st["n_edges"] == len(want), (o.name, how)       # length-gated pairs are no alignments
    return let_through


def _both_ways(o, tmp_path):
    (al1, ed1, st1), (al2, ed2, st2) = _runs(o, tmp_path)
    n = _check(o, al1, ed1, st1, "one align() call")
    _check(o, al2, ed2, st2, "one align() call per query")
    assert al1.tobytes() == al2.tobytes()
    # the sharing did happen: every pair has its mirror in the list, so the one call ran fewer DPs than the calls that see one direction each
    if n >= 2:
        assert st1["n_sw_runs"] < st2["n_sw_runs"], (o.name, st1["n_sw_runs"], st2["n_sw_runs"])
    return st1, st2


@pytest.mark.parametrize("o", G.OPTION_SETS["cov"], ids=repr)
def test_coverage_gate(o, tmp_path):
    """finalize_kernel: spans round(c L) + {-1, 0, 1} of L under --cov-mode 0 / 1 / 2, the boundary on qcov alone, tcov alone and both"""
    _both_ways(o, tmp_path)


@pytest.mark.parametrize("o", G.OPTION_SETS["len"], ids=repr)
def test_length_gate(o, tmp_path):
    """len_gate_kernel: the same grid as sequence lengths, related and unrelated pairs, a 1-residue sequence; a gated pair keeps the
    all-zero record, is no alignment and adds no cells; off under -c 0"""
    st1, st2 = _both_ways(o, tmp_path)
    g = o.group()
    cells = sum(pr["lq"] * pr["lt"] for pr in g.pairs if G.length_gate_lets_through(o, pr["lq"], pr["lt"]))
    assert st1["cells_fwd"] == cells and st2["cells_fwd"] == cells


@pytest.mark.parametrize("o", G.OPTION_SETS["sid"], ids=repr)
def test_identity_gate(o, tmp_path):
    """tb_apply_kernel and, for the mirrors, tbm_resolve_kernel: identities round(s k) + {-1, 0, 1} of k columns, with and without a gap"""
    _both_ways(o, tmp_path)


@pytest.mark.parametrize("o", G.OPTION_SETS["eval"], ids=repr)
def test_evalue_gate(o, tmp_path):
    """gate_kernel, both passes, with per-query thresholds corrected, corrected + 1, score, score + 1: the last fails without a reversed
    pass (score_rev 0); the two directions of a pair pass and fail in all four combinations"""
    st1, st2 = _both_ways(o, tmp_path)
    if o.table == "none":          # nothing reaches its threshold: the forward pass alone ran, once per unordered pair
        n = len(o.group().pairs)
        assert (st1["n_sw_runs"], st2["n_sw_runs"]) == (n // 2, n) and st1["n_start_alignments"] == 0


@pytest.mark.parametrize("o", G.OPTION_SETS["routes"], ids=repr)
def test_routes(o, tmp_path):
    """the same gate kernels behind the int32 kernels, the long-query kernel and the int32 re-run of a score past the packed range"""
    st1, st2 = _both_ways(o, tmp_path)
    if o.name.startswith("ovf"):
        assert st1["n_pk_reruns"] >= len(o.group().pairs) // 2 and st2["n_pk_reruns"] >= len(o.group().pairs)


def test_set_hits_refuses_a_list_that_names_a_target_twice():
    """(q, t), (q, t) in one list would be keyed as a pair and its mirror and the second entry given a transposed record: UC_ERR_ARGS, naming
    query and target; the list installed before stays in place"""
    import unicore_amd as U
    o = G.OPTION_SETS["cov"][0]
    g = o.group()
    e = U.Engine(o.opts(), verbosity=1)
    e.set_db(*util.flat(g.s3, g.sa))
    hits = np.zeros(len(g.pairs), U.HIT_DTYPE)
    hits["target"] = g.t
    e.set_hits(g.counts, hits)
    e.align()
    before = e.alns().copy()
    q = int(np.nonzero(g.counts >= 2)[0][0])
    k = int(g.counts[:q].sum())
    twice = hits.copy()
    twice["target"][k + 1] = twice["target"][k]
    with pytest.raises(U.UcError) as x:
        e.set_hits(g.counts, twice)
    assert x.value.code == U.UC_ERR_ARGS
    assert "query %d " % q in str(x.value) and "target %d " % twice["target"][k] in str(x.value), str(x.value)
    cnt, kept = e.hits()
    assert np.array_equal(cnt, g.counts) and np.array_equal(kept["target"], g.t)
    e.align()
    assert e.alns().tobytes() == before.tobytes()
    # the same target in the lists of two queries is what every database has
    shared = np.zeros(2, U.HIT_DTYPE)
    shared["target"] = 1
    cnt2 = np.zeros(len(g.s3), np.uint32)
    cnt2[[0, 2]] = 1
    e.set_hits(cnt2, shared)
    e.align()
    assert len(e.alns()) == 2
    e.close()
