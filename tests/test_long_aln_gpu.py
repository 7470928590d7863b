"""Traceback statistics of alignments of 32,768 columns and more on the GPU (cases and references: tests/long_aln_cases.py).

Kernel level: every producer of (alignment length, identities, gaps) - packed MODE 7 + the byte walk (banded, whole box), int32 MODE 3
of the systolic classes and of the long-query kernel, the emitting walks of -a on all four routes - on the reference's boxes and scores.
Pipeline level: Engine.align on both orders of every pair under a --min-seq-id on either side of the reference identity, every record
field; one search + convertalis, m8 bytes.

The default-cost (nat) pairs run MODE 3 and one align; they do not run -a: their stored int32 matrix would be 4.3 GB and
tb_plain_dp_kernel is one workgroup per pair.  The -a routes are covered by the free-extension cases, whose matrices are 26 to 550 MB.

Before the fix.  This module ran once on the parent's kernels, when one 32-bit word held length << 16 | identities | tie << 31.  Red:
every case with 32,768 columns or more, in every test that reaches it, with exactly the numbers the layout predicts - z-walk-32768,
z-long-32768 and nat-32768 came back with length 0, tie-z (32,769) with 1, nat-mutated (33,185) with 417, z-wide (65,644 / 65,629) with 108
/ 93; identities and gaps were right; the search's m8 row read fident 0.000, alnlen 0, mismatch 32768.  Green: every 32,767 case and
tie-small, at kernel level.  (The align test was red for those too, for a reason of the test: it compared the gap count, which the
cluster path does not compute.  It now compares it where the engine computes it, under -a.)  One expectation did not hold and is
dropped: no pair of these shapes can leave its stored band, see test_mode7_whole_box_and_banded.

Time, measured on one MI355X: the module takes 37 s, of which 8.5 s are the CPU references of the z group and 12 s the two nat tests;
test_sw_kernels.py, the comparable module, takes 8 s.  A MODE 3 pass over a 32,768 x 32,768 box takes 1.9 s (the long-query kernel
gives a pair one wave: 0.55 G cells/s, five times the 0.4 s estimated from instruction counts), a score pass 0.38 s.  Pairs run side by
side, so the nat tests' 6 s each are the time of their passes over ONE such box - three MODE 3 passes; five score passes and two MODE 3
passes - and leaving out the mutated pair would not shorten them; the 32,767 / 32,768 boundary itself sets the time.
"""
import numpy as np
import pytest

import bt_ref
import long_aln_cases as L
import util

pytestmark = pytest.mark.gpu

STATS = ("aln_len", "idents", "gaps")
SYS_ROWS = 2048                 # queries of more rows take the long-query kernel


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _group(cases):
    """one database of the cases' sequences and both orders of every pair with their reference"""
    s3, sa, pairs = [], [], []
    for c in cases:
        i = len(s3)
        s3 += [c["q"][0], c["t"][0]]; sa += [c["q"][1], c["t"][1]]
        for order, (a, b) in enumerate(((i, i + 1), (i + 1, i))):
            rec, tie = c["ref"][order]
            pairs.append(dict(name=c["name"], order=order, q=a, t=b, rec=rec, tie=tie))
    g = dict(s3=s3, sa=sa, pairs=pairs, opts=cases[0]["opts"])
    g["q"] = np.array([x["q"] for x in pairs], np.uint32); g["t"] = np.array([x["t"] for x in pairs], np.uint32)
    g["box"] = np.array([[x["rec"][f] for f in ("qstart", "qend", "tstart", "tend")] for x in pairs], np.int32)
    g["known"] = np.array([x["rec"]["score"] for x in pairs], np.int32)
    g["want"] = np.array([[x["rec"]["aln_len"], x["rec"]["idents"], x["rec"]["gap_opens"]] for x in pairs], np.int32)
    g["rows"] = np.array([len(s3[x["q"]]) for x in pairs])
    g["label"] = ["%s/%d" % (x["name"], x["order"]) for x in pairs]
    return g


@pytest.fixture(scope="module", params=[L.Z_OPTS, L.TIEZ_OPTS, L.TIE_OPTS], ids=["z", "tie-z", "tie-small"])
def group(request):
    return _group([L.z_case(n) for n, (o, _) in L.Z_CASES.items() if o == request.param])


@pytest.fixture(scope="module")
def nat():
    return _group([L.nat_case(n) for n in L.NAT_CASES])


def _engine(g, extra=""):
    import unicore_amd as U
    e = U.Engine(("-c 0 " + extra + " " + g["opts"]).strip(), verbosity=1)
    e.set_db(*util.flat(g["s3"], g["sa"]))
    return e


def _equal(g, r, sel=None):
    """(aln_len, idents, gaps) of the selected pairs equal the reference; every difference is named"""
    idx = np.arange(len(g["q"])) if sel is None else np.nonzero(sel)[0]
    got = np.stack([r[f] for f in STATS], axis=1)
    bad = ["%s: got %s, reference %s" % (g["label"][i], got[k].tolist(), g["want"][i].tolist()) for k, i in enumerate(idx)
           if not np.array_equal(got[k], g["want"][i])]
    assert not bad, "\n".join(bad)


def _pass(e, g, tab, mode, sel=None, **kw):
    s = np.ones(len(g["q"]), bool) if sel is None else sel
    return e.sw_pass(tab, mode, g["q"][s], g["t"][s], box=g["box"][s], known=g["known"][s] if mode == 7 else None, **kw)


def test_mode7_whole_box_and_banded(group):
    """table 1 MODE 7: packed classes store H bytes and walk them, longer queries take MODE 3 of the long-query kernel.  Through the
    library's routing (whole box, band of 48) and raw.  No pair here can leave its band: the band spans the diagonals between the box's
    corners, and a box of a packed class (at most 2,048 rows) with 32,768 columns of alignment is at least 30,720 columns wider than
    tall, so tb_band_of stores the whole box whatever W is.  The band-miss word (TB_BAND_MISS) therefore never meets a long alignment;
    its route is tested where it occurs (test_backtrace_gpu.py, test_sw_kernels.py)."""
    e = _engine(group)
    for W in (0, 48):
        _equal(group, _pass(e, group, 1, 7, band=W))
    r = _pass(e, group, 1, 7, band=1, raw=True)
    miss = r["miss"] != 0
    assert not miss[group["want"][:, 0] >= L.LIMIT15 - 1].any()
    _equal(group, {f: r[f][~miss] for f in STATS}, ~miss)


def test_mode3_systolic_classes_and_long_query_kernel(group):
    e = _engine(group)
    r = _pass(e, group, 2, 3)
    _equal(group, r)
    long_cls = r["cls"].max()
    if (group["rows"] > SYS_ROWS).any():
        assert ((r["cls"] == long_cls) == (group["rows"] > SYS_ROWS)).all()
    # the all-int32 configuration takes the same kernels through the library's routing
    e2 = _engine(group, "--sw-kernel i32")
    _equal(group, e2.sw_pass(2, 3, group["q"], group["t"], box=group["box"]))


def _check_cigars(g, r, sel):
    for k, i in enumerate(np.nonzero(sel)[0]):
        runs = bt_ref.parse(r["cigar"][k])
        ops = [op for _, op in runs]
        n = {o: sum(c for c, op in runs if op == o) for o in "MID"}
        ln, idn, gaps = (int(x) for x in g["want"][i])
        qs, qe, ts, te = (int(x) for x in g["box"][i])
        assert n["M"] + n["I"] + n["D"] == ln, g["label"][i]
        assert (n["M"] + n["I"], n["M"] + n["D"]) == (qe - qs + 1, te - ts + 1), g["label"][i]
        assert sum(op != "M" for op in ops) == gaps and n["M"] >= idn, g["label"][i]
        assert all(a != b for a, b in zip(ops, ops[1:])) and ops[0] == "M" and ops[-1] == "M", g["label"][i]
        assert gaps - sum(a != "M" and b != "M" for a, b in zip(ops, ops[1:])) + 1 == ops.count("M"), g["label"][i]


def test_emitting_walks_on_every_route(group):
    """-a: route 0 banded bytes, 1 whole-box bytes (packed classes), 2 stored int32 matrix (any pair; z-wide's 550 MB matrix is left to
    route 3, one order), 3 the long-query route.  Statistics equal the reference; the CIGAR's runs sum to the reference length and the
    box, its gap runs are the reference's gaps, and its M runs are what separates them"""
    g = group
    e = _engine(g)
    packed, wide = g["rows"] <= SYS_ROWS, np.array([x["name"] == "z-wide" for x in g["pairs"]])
    first = np.array([x["order"] == 0 for x in g["pairs"]])
    plan = [(1, packed, 0), (2, ~wide, 0), (3, ~packed & (~wide | first), 0)]
    for route, sel, band in plan:
        if not sel.any():
            continue
        r = e.tb_emit_pass(route, g["q"][sel], g["t"][sel], g["box"][sel], g["known"][sel], band=band)
        assert not r["miss"].any() and ((r["plain"] != 0).all() if route >= 2 else not r["plain"].any())
        _equal(g, r, sel)
        _check_cigars(g, r, sel)
    r = e.tb_emit_pass(0, g["q"][packed], g["t"][packed], g["box"][packed], g["known"][packed], band=48)
    miss = r["miss"] != 0
    keep = packed.copy(); keep[np.nonzero(packed)[0][miss]] = False
    _equal(g, {f: r[f][~miss] for f in STATS}, keep)
    _check_cigars(g, dict(cigar=[c for c, m in zip(r["cigar"], miss) if not m]), keep)
    assert all(c == "" for c, m in zip(r["cigar"], miss) if m)


def _align(g, x, extra=""):
    """Engine.align of the group's pairs (both orders are in the list: mutual hits) under --min-seq-id x -> records in pair order"""
    e = _engine(g, "--min-seq-id %s %s" % (x, extra))
    order = np.lexsort((g["t"], g["q"]))
    cnt = np.bincount(g["q"], minlength=e.n).astype(np.uint32)
    import unicore_amd as U
    hits = np.zeros(len(order), U.HIT_DTYPE)
    hits["target"] = g["t"][order]
    e.set_hits(cnt, hits)
    e.align()
    al = e.alns()
    out = np.zeros_like(al)
    out[order] = al
    return out


def _check_records(g, al, x, gaps=False):
    """every field of every record; the gap count is part of a record only where the engine computes it (the search path and -a)"""
    bad, accepted = [], []
    for i, pr in enumerate(g["pairs"]):
        want = dict(pr["rec"])
        want["accepted"] = int(L.seq_id(want) >= np.float32(x))
        accepted.append(want["accepted"])
        got = {f: int(al[f][i]) for f in L.FIELDS}
        if not gaps:
            assert got["gap_opens"] == 0
            got["gap_opens"] = want["gap_opens"]
        if got != want:
            bad.append("%s under --min-seq-id %s:\n  got       %s\n  reference %s" % (g["label"][i], x, got, want))
    assert not bad, "\n".join(bad)
    return accepted


def test_align_both_orders_on_either_side_of_the_identity(group):
    """every field of every record, each order against its own reference (z-wide and the tie cases have a tie mark: the mirror
    must not copy its partner), accepted under the lower threshold and rejected under the upper; without the sharing of mutual hits;
    with -a, which also computes the gap count"""
    lo, hi = L.GROUP_SEQ_IDS[group["opts"]]
    assert all(_check_records(group, _align(group, lo), lo))
    assert not any(_check_records(group, _align(group, hi, "--sym-dedup 0"), hi))
    assert all(_check_records(group, _align(group, lo, "-a"), lo, gaps=True))


def test_search_and_convertalis_m8_bytes(O, tmp_path):
    """the search path computes all three statistics; BLAST-tab alnlen, fident, mismatch and gapopen equal the oracle's writer's"""
    import unicore_amd as U
    c = L.z_case("z-long-32768")
    opts = "-c 0 " + L.Z_OPTS
    qdbp, tdbp, out = str(tmp_path / "q"), str(tmp_path / "t"), str(tmp_path / "res")
    util.write_db(qdbp, [c["q"][0]], [c["q"][1]], ["query_0"])
    util.write_db(tdbp, [c["t"][0]], [c["t"][1]], ["target_0"])
    U.search(qdbp, tdbp, out + "_aln", str(tmp_path / "tmp"), opts, threads=4)
    U.convertalis(qdbp, tdbp, out + "_aln", out + ".m8")
    qdb, tdb = O.OracleDb(qdbp), O.OracleDb(tdbp)
    po = util.oracle_params(O, "-e 10 --max-seqs 1000 " + opts)
    O.write_m8(out + "_ref.m8", qdb, tdb, po, O.search(qdb, tdb, po, threads=4))
    got, exp = open(out + ".m8", "rb").read(), open(out + "_ref.m8", "rb").read()
    assert got == exp, (got, exp)
    rows = [l.split("\t") for l in got.decode().splitlines()]
    assert len(rows) == 1 and (int(rows[0][3]), int(rows[0][4]), int(rows[0][5])) == (L.LIMIT15, 0, 1)


def test_nat_pairs_mode3(nat):
    """default gap costs, boxes of 32,767^2 to 33,000^2 cells and scores far beyond the packed range: int32 MODE 3 of the long-query
    kernel, one order of each pair, the three pairs side by side in each of the three passes (length, identities, gaps)"""
    e = _engine(nat)
    first = np.array([x["order"] == 0 for x in nat["pairs"]])
    r = _pass(e, nat, 2, 3, sel=first)
    _equal(nat, r, first)
    assert (r["cls"] == r["cls"][0]).all()


def test_nat_pairs_align(nat):
    """ONE align run of both orders against the fixture's records, under the upper of the fixture's thresholds: the identical pairs
    pass, the mutated pair (identity 0.72) is rejected"""
    hi = L.NAT_SEQ_IDS[1]
    acc = _check_records(nat, _align(nat, hi), hi)
    assert acc == [0 if pr["name"] == "nat-mutated" else 1 for pr in nat["pairs"]]
