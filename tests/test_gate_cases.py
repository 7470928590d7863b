"""The reference side of the gate-threshold tests (tests/gate_cases.py): every shipped pair has the alignment it was built for, the
closed-form expectation equals the scalar oracle and the SIMD leg under every option set the GPU test runs, and the table of cases can tell
the spec's float rule from its near misses and reaches every branch of the mutual-hit sharing."""
import collections

import numpy as np
import pytest

import gate_cases as G
import util


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _all_groups():
    return ([G.cov_group(c) for c in G.COV_THRESHOLDS] + [G.sid_group(s) for s in G.SID_THRESHOLDS] + [G.len_group(c) for c in G.LEN_THRESHOLDS] +
            [G.eval_group(), G.long_group(), G.ovf_group()])


def test_the_matrices_allow_the_construction():
    S3, SA = G.matrices()
    ln = G.letters()
    assert (S3 == S3.T).all() and (SA == SA.T).all()                     # mutual hits share a DP only then
    assert ln["worst"] == S3.min() + SA.min() and ln["worst"] < -G.base_params().gap_open
    assert np.diag(S3).min() > 0 and np.diag(SA).min() > 0             # an end column of a core scores > 0
    off = SA + 100 * np.eye(20, dtype=np.int64)
    assert np.diag(S3).min() + off.min() >= 0                            # a substituted AA letter leaves its column at >= 0
    # the three untouched columns on either side of the deletion outweigh the gap
    assert 3 * (np.diag(S3).min() + np.diag(SA).min()) > G.base_params().gap_open + (G.GAP - 1) * G.base_params().gap_ext
    assert (G.OVF_L * G.OVF_C - 1) * ln["best_score"] - 2 * 40 >= G.PK_LIMIT


# pairs with an intent per family over all groups, pairs without (unrelated sequences), and generator attempts that did not land
# (four pairs per grid point: 120, 119, 117, 110, 120, 128 and 80 points at the seven coverage thresholds, 3 + 3 on the two routes)
PINNED_PAIRS = {"cov": 3176 + 12 + 12, "len-related": 480 + 512, "sid": 1208 + 12, "eval": 96}
PINNED_UNRELATED = 2 * (120 + 3) + 2 * (128 + 3)
PINNED_RETRIES = 0


def test_every_shipped_case_lands(O):
    """the scalar oracle at threshold 1 gives exactly the intended ends, starts, alignment length, identities and gaps, and the score the
    numpy sum over the core's columns (minus one gap of three) gives"""
    p = G.base_params()
    n, unrelated, bad = collections.Counter(), 0, []
    for g in _all_groups():
        odb = O.OracleDb(s3=g.s3, sa=g.sa)
        for pr in g.pairs:
            if pr["want"] is None:
                unrelated += 1
                continue
            r = O.align_pair(odb, p, pr["q"], pr["t"], 1)
            got = {f: int(r[f]) for f in pr["want"]}
            if got != pr["want"] or int(r["pass_evalue"]) != 1 or int(r["score_rev"]) != pr["rev"] or pr["rev"] <= 0:
                bad.append("%s: got %s, intended %s" % (pr["label"], got, pr["want"]))
            n[pr["family"]] += 1
    assert not bad, "\n".join(bad[:10])
    assert dict(n) == PINNED_PAIRS and unrelated == PINNED_UNRELATED, (dict(n), unrelated)
    assert sum(g.attempts for g in _all_groups()) == PINNED_RETRIES


def test_routes_reach_what_they_are_named_for():
    lg, og = G.long_group(), G.ovf_group()
    assert sum(pr["lq"] > G.SYS_ROWS for pr in lg.pairs) >= 8 and all(2049 <= max(pr["lq"], pr["lt"]) <= 2100 for pr in lg.pairs)
    assert all(pr["want"]["score"] >= G.PK_LIMIT and max(pr["lq"], pr["lt"]) <= G.SYS_ROWS for pr in og.pairs)
    assert {(pr["want"]["qend"] - pr["want"]["qstart"] + 1, G.OVF_L) for pr in og.pairs} == {(1699, 2000), (1700, 2000), (1701, 2000)}


@pytest.mark.parametrize("o", G.ALL_SETS, ids=repr)
def test_closed_form_equals_the_oracle(o):
    """every field of every record; only unrelated sequences that the length gate lets through have no closed form"""
    g, thr, ora = o.group(), G.thresholds(o, o.group()), G.oracle_records(o)
    bad, unknown = [], 0
    for i, pr in enumerate(g.pairs):
        exp = G.expected(o, pr, int(thr[pr["q"]]))
        if exp is None:
            assert pr["family"] == "len-unrelated"
            unknown += 1
        elif G.normalised(exp) != ora[i]:
            bad.append("%s under %s:\n  closed form %s\n  oracle      %s" % (pr["label"], o.opts(), G.normalised(exp), ora[i]))
    assert not bad, "\n".join(bad[:10])
    assert unknown < len(g.pairs)


@pytest.mark.parametrize("o", G.ALL_SETS, ids=repr)
def test_simd_leg_equals_the_oracle(O, o):
    g = o.group()
    p = util.oracle_params(O, o.opts())
    tab = np.ascontiguousarray(G.thresholds(o, g), np.int32)
    if o.table:
        p.min_score_table = tab.ctypes.data
    got = O.simd_align_pairs(O.OracleDb(s3=g.s3, sa=g.sa), p, np.stack([g.q, g.t], axis=1), threads=4)
    bad = ["%s: simd %s, scalar %s" % (pr["label"], G.normalised(got[i]), ref) for i, (pr, ref) in enumerate(zip(g.pairs, G.oracle_records(o)))
           if G.normalised(got[i]) != ref]
    assert not bad, "\n".join(bad[:10])


def _points(g):
    """(numerator, denominator) of every quotient a gate forms on the group's intended records"""
    cov, sid, ln = set(), set(), set()
    for pr in g.pairs:
        ln.add((pr["lq"], pr["lt"]))
        w = pr["want"]
        if w is not None:
            cov |= {(w["qend"] - w["qstart"] + 1, pr["lq"]), (w["tend"] - w["tstart"] + 1, pr["lt"])}
            sid.add((w["idents"], w["aln_len"]))
    return cov, sid, ln


def _misses(points, thr):
    d = {(a, b) for a, b in points if G.f32_ge(a, b, thr) != G.double_ge(a, b, thr)}
    r = {(a, b) for a, b in points if G.f32_ge(a, b, thr) != G.recip_ge(a, b, thr)}
    return d, r


def test_the_table_tells_the_rule_from_its_near_misses():
    """per threshold, the shipped quotients on which (i) a division in double, (ii) a multiplication with the rounded reciprocal decides
    differently from the float rule.  The floors are conditions on the table: ten of (i) wherever the float of the threshold differs from
    the decimal, two of (ii) everywhere, four at 0.5 (its added lengths)"""
    for c in G.COV_THRESHOLDS:
        d, r = _misses(_points(G.cov_group(c))[0], c)
        print("cov %s: (i) %d (ii) %d" % (c, len(d), len(r)))
        assert len(d) >= (10 if c not in (0.5, 1.0) else 0) and len(r) >= (4 if c == 0.5 else 2), c
    d, r = _misses(_points(G.cov_group(0.8))[0], 0.8)
    assert (4, 5) in d and (8, 10) in d and (20, 25) in r and (40, 50) in r          # the cases a reviewer's scratch build turns red
    for c in G.LEN_THRESHOLDS:                       # the length gate reads the same grid as (Lq, Lt), in related and unrelated pairs
        lens = _points(G.len_group(c))[2]
        unrelated = {(pr["lq"], pr["lt"]) for pr in G.len_group(c).pairs if pr["want"] is None}
        for pts in (lens, unrelated):
            d, r = _misses(pts, c)
            assert len(d) >= (10 if c != 0.5 else 0) and len(r) >= (4 if c == 0.5 else 2), c
    for s in G.SID_THRESHOLDS:                       # 0.9 and 1.0: the float is not above the decimal, a double quotient decides alike
        d, r = _misses(_points(G.sid_group(s))[1], s)
        print("sid %s: (i) %d (ii) %d" % (s, len(d), len(r)))
        assert len(d) >= (10 if s in (0.6, 0.3, 0.2) else 0) and len(r) >= (2 if s in (0.6, 0.3, 0.2) else 0), s
    assert float(np.float32(0.9)) < 0.9 and float(np.float32(0.6)) > 0.6 and float(np.float32(0.8)) > 0.8


def test_every_threshold_accepts_and_rejects():
    """no option set passes or fails everything (but the two that are meant to), and wherever the grid is not clipped the three spans
    around round(c L) hold an accepted and a rejected one"""
    for o in G.ALL_SETS:
        acc = {r["accepted"] for r in G.oracle_records(o)}
        assert acc == ({0} if o.name == "eval-none" else {0, 1}), o
        if o.len_gate:
            gated = [not G.length_gate_lets_through(o, pr["lq"], pr["lt"]) for pr in o.group().pairs]
            assert (any(gated) and not all(gated)) if o.c > 0 else not any(gated), o
    for c in G.COV_THRESHOLDS:
        for L in G.GRID_L:
            ks = [G.rnd(c * L) + d for d in (-1, 0, 1)]
            if ks[0] >= 3 and ks[2] <= L:
                assert {G.f32_ge(k, L, c) for k in ks} == {False, True}, (c, L)
    for s in G.SID_THRESHOLDS:
        for k in G.SID_K:
            idn = {k - m - (G.GAP if gapped else 0) for m, gapped in G.sid_variants(s, k)}
            if G.rnd(s * k) - 1 >= 2:          # (0.2 at k = 7 and 10: one identity would take a substitution in an end column)
                assert {G.f32_ge(i, k, s) for i in idn} == {False, True}, (s, k)


def _combos(o, field):
    """over the mutual pairs of an option set: (value of `field` in the direction the engine computes, in its mirror) -> count"""
    g, ora = o.group(), G.oracle_records(o)
    n = collections.Counter()
    for i, pr in enumerate(g.pairs):
        if pr["rep"] and pr["mirror"] is not None:
            n[(int(ora[i][field] > 0), int(ora[pr["mirror"]][field] > 0))] += 1
    return dict(n)


def test_mutual_hits_reach_every_branch():
    """every pair with an intent is listed in both directions; with the table, and under --cov-mode 1 / 2, the shared DP's owner and its
    mirror pass and fail in all four combinations"""
    for g in _all_groups():
        assert all(pr["mirror"] is not None for pr in g.pairs)
    sets = {o.name: o for o in G.ALL_SETS}
    # X passes only with the threshold `corrected`, runs the reversed pass with all but `score+1`; the same for Y, independently
    assert _combos(sets["eval-mixed-mode0"], "pass_evalue") == {(1, 1): 3, (1, 0): 9, (0, 1): 9, (0, 0): 27}
    assert _combos(sets["eval-mixed-mode0"], "score_rev") == {(1, 1): 27, (1, 0): 9, (0, 1): 9, (0, 0): 3}
    assert _combos(sets["eval-none"], "score_rev") == {(0, 0): 48}
    for c in G.COV_THRESHOLDS:
        one, two = _combos(sets["cov-%s-mode1" % c], "accepted"), _combos(sets["cov-%s-mode2" % c], "accepted")
        # the bare core as query is always covered, as target it always covers: under mode 2 the owner (the shorter query) passes
        # alone, under mode 1 its mirror does
        assert one.get((0, 1), 0) > 0 and two.get((1, 0), 0) > 0 and one.get((1, 0), 0) == 0 and two.get((0, 1), 0) == 0, c
        for n in (one, two):
            assert n.get((1, 1), 0) > 0 and n.get((0, 0), 0) > 0, c
