"""Alignment backtraces (-a) on the GPU: every traceback route through the kernel-level entry point against the tests' restatement of the
oracle's traceback (tests/bt_ref.py), string for string; then uc_search / convertalis / unicore search / uc_cluster and the staged API
(mutual hits) with -a."""
import os
import subprocess

import numpy as np
import pytest

import bt_ref
import util
from test_backtrace import EXTREME

pytestmark = pytest.mark.gpu

CAPS1 = [32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 448, 512, 576, 640, 704, 768, 896, 1024, 1152, 1280, 1408, 1536,
         1664, 1792, 1920, 2048]                 # query rows of the packed classes (table 1)
BANDS = (0, 1, 4, 48)
SW_PK_OVF = 0x7C00 - 256


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _reference(O, p, s3, sa, pairs):
    """boxes, scores and the restatement's (len, idents, gaps, cigar) of every pair; no pair is dropped"""
    S3, SA = bt_ref.matrices(p)
    box, known, want = [], [], []
    for q, t in pairs:
        b = bt_ref.box_of(O, p, s3[q], sa[q], s3[t], sa[t])
        assert b is not None, (q, t)
        s, qs, qe, ts, te = b
        r = bt_ref.traceback(s3[q][qs:qe + 1], sa[q][qs:qe + 1], s3[t][ts:te + 1], sa[t][ts:te + 1], S3, SA, p.gap_open, p.gap_ext)
        assert r[4] == s
        box.append((qs, qe, ts, te)); known.append(s); want.append(r[:4])
    return np.array(box, np.int32), np.array(known, np.int32), want


def _same(r, want, sel=None):
    for i, w in enumerate(want):
        if sel is not None and not sel[i]:
            continue
        assert (r["aln_len"][i], r["idents"][i], r["gaps"][i], r["cigar"][i]) == w, (i, w, r["cigar"][i])


@pytest.fixture(scope="module")
def material(O):
    p = O.default_params()
    rng = np.random.default_rng(77)
    lengths = sorted({c for c in CAPS1} | {c - 9 for c in CAPS1 if c > 32} | {1, 5, 33})
    s3, sa, pr = bt_ref.pair_set(rng, lengths)
    pr = [x for x in pr if O.sw(s3[x[0]], sa[x[0]], s3[x[1]], sa[x[1]], p)[0] > 0]      # a box needs a positive score (one-residue sequences)
    pairs = [(q, t) for q, t, _ in pr]
    kinds = np.array([k for _, _, k in pr])
    box, known, want = _reference(O, p, s3, sa, pairs)
    return dict(p=p, s3=s3, sa=sa, pairs=pairs, kinds=kinds, box=box, known=known, want=want)


def _engine(opts, s3, sa):
    import unicore_amd as U
    e = U.Engine(opts, verbosity=1)
    e.set_db(*util.flat(s3, sa))
    return e


def test_packed_routes_every_class_every_band(material):
    """table 1 MODE 7 + emitting walk: all 28 classes, W = 0 / 1 / 4 / 48 and the whole-box route; W never changes a string, a pair that
    leaves its band has no string and gets it from the whole-box redo"""
    M = material
    e = _engine("-c 0.8", M["s3"], M["sa"])
    q = np.array([a for a, _ in M["pairs"]], np.uint32); t = np.array([b for _, b in M["pairs"]], np.uint32)
    whole = e.tb_emit_pass(1, q, t, M["box"], M["known"])
    _same(whole, M["want"])
    assert set(whole["cls"].tolist()) == set(range(28)) and not whole["plain"].any() and not whole["miss"].any()
    missed = np.zeros(len(q), bool)
    for W in BANDS:
        r = e.tb_emit_pass(0, q, t, M["box"], M["known"], band=W)
        miss = r["miss"] != 0
        assert not r["plain"].any() and (W > 0 or not miss.any())
        _same(r, M["want"], ~miss)
        assert all(r["cigar"][i] == "" for i in np.nonzero(miss)[0])
        missed |= miss
    assert (missed & (M["kinds"] == "zigzag")).any()                 # the band-miss route ran ...
    redo = np.nonzero(missed)[0]
    r = e.tb_emit_pass(1, q[redo], t[redo], M["box"][redo], M["known"][redo])
    _same(r, [M["want"][i] for i in redo])                           # ... and its whole-box redo gives the same strings


def test_stored_matrix_route_on_every_pair_and_int32_configuration(material):
    M = material
    q = np.array([a for a, _ in M["pairs"]], np.uint32); t = np.array([b for _, b in M["pairs"]], np.uint32)
    for opts in ("-c 0.8", "-c 0.8 --sw-kernel i32"):
        e = _engine(opts, M["s3"], M["sa"])
        r = e.tb_emit_pass(2, q, t, M["box"], M["known"])
        assert r["plain"].all()
        _same(r, M["want"])


def test_extreme_matrices_take_the_stored_matrix(O):
    """+-48 matrices with --gap-open 31: neighbouring cells differ by more than a byte holds, the walk reads int32 cells"""
    p = util.oracle_params(O, EXTREME)
    rng = np.random.default_rng(5)
    s3, sa, pr = bt_ref.pair_set(rng, [1, 40, 150, 333, 700])
    pairs = [(q, t) for q, t, _ in pr if O.sw(s3[q], sa[q], s3[t], sa[t], p)[0] > 0]
    box, known, want = _reference(O, p, s3, sa, pairs)
    e = _engine("-c 0.8 " + EXTREME, s3, sa)
    q = np.array([a for a, _ in pairs], np.uint32); t = np.array([b for _, b in pairs], np.uint32)
    r = e.tb_emit_pass(2, q, t, box, known)
    assert r["plain"].all()
    _same(r, want)


def test_long_query_route(O):
    p = O.default_params()
    rng = np.random.default_rng(9)
    a = bt_ref._rnd(rng, 2300); z = bt_ref.zigzag(rng, 2100)
    b = bt_ref.mutate(rng, a[0], a[1], 0.2)
    s3, sa = [a[0], b[0], z[0][0], z[1][0]], [a[1], b[1], z[0][1], z[1][1]]
    assert len(s3[0]) > 2048 and len(s3[2]) > 2048
    pairs = [(0, 1), (2, 3)]
    box, known, want = _reference(O, p, s3, sa, pairs)
    e = _engine("-c 0.8", s3, sa)
    r = e.tb_emit_pass(3, np.array([0, 2], np.uint32), np.array([1, 3], np.uint32), box, known, band=48)
    assert r["plain"].all() and (r["cls"] == 28).all()
    _same(r, want)


def test_scores_beyond_the_packed_range(O, tmp_path):
    """the scaled-matrix construction of test_packed_range_edge: self and near-self pairs whose scores pass SW_PK_OVF"""
    from test_sw_kernels import _scaled_matrix
    m3 = str(tmp_path / "m3.out")
    _scaled_matrix(os.path.join(util.ROOT, "unicore_amd", "data", "mat3di_synthetic.out"), m3, 4)
    p = O.default_params()
    assert O.lib().uco_load_matrix(m3.encode(), p.S3) == 0
    rng = np.random.default_rng(3)
    s3, sa, pairs = [], [], []
    for L in (1500, 2000):
        a = bt_ref._rnd(rng, L)
        b = bt_ref.mutate(rng, a[0], a[1], 0.03)
        s3 += [a[0], b[0]]; sa += [a[1], b[1]]
        pairs += [(len(s3) - 2, len(s3) - 1), (len(s3) - 2, len(s3) - 2)]
    box, known, want = _reference(O, p, s3, sa, pairs)
    assert (known >= SW_PK_OVF).all()
    e = _engine("-c 0.8 --mat3di %s" % m3, s3, sa)
    q = np.array([a for a, _ in pairs], np.uint32); t = np.array([b for _, b in pairs], np.uint32)
    r = e.tb_emit_pass(2, q, t, box, known)
    assert r["plain"].all()
    _same(r, want)


# ---- engine, on-disk, CLI -----------------------------------------------------------------------------------------------------
def _read_aln_db(prefix):
    data = open(prefix, "rb").read()
    rows = {}
    for line in open(prefix + ".index"):
        k, off, ln = (int(x) for x in line.split())
        rows[k] = [r.split("\t") for r in data[off:off + ln].rstrip(b"\0").decode().splitlines()]
    return rows


@pytest.fixture(scope="module")
def dbs(tmp_path_factory):
    d = tmp_path_factory.mktemp("btdb")
    s3q, saq = util.family_db(21, n_fam=10, members=5, extra=(700, 2300))
    rng = np.random.default_rng(4)
    s3t = [bt_ref.mutate(rng, a, b, 0.1)[0] for a, b in zip(s3q, saq)]
    rng = np.random.default_rng(4)
    sat = [bt_ref.mutate(rng, a, b, 0.1)[1] for a, b in zip(s3q, saq)]
    s3t += s3q[:20]; sat += saq[:20]
    qdb, tdb = str(d / "q"), str(d / "t")
    util.write_db(qdb, s3q, saq, names=["q%d" % i for i in range(len(s3q))])
    util.write_db(tdb, s3t, sat, names=["t%d" % i for i in range(len(s3t))])
    return dict(dir=str(d), qdb=qdb, tdb=tdb, s3q=s3q, saq=saq, s3t=s3t, sat=sat)


def _check_rows(O, dbs, rows, opts):
    p = util.oracle_params(O, opts)
    S3, SA = bt_ref.matrices(p)
    n = 0
    for qk, rr in rows.items():
        for f in rr:
            assert len(f) == 15
            t, qs, qe, ts, te, alen, idn, gaps = int(f[0]), int(f[4]), int(f[5]), int(f[7]), int(f[8]), int(f[10]), int(f[11]), int(f[12])
            q3, qa = dbs["s3q"][qk][qs:qe + 1], dbs["saq"][qk][qs:qe + 1]
            t3, ta = dbs["s3t"][t][ts:te + 1], dbs["sat"][t][ts:te + 1]
            want = bt_ref.traceback(q3, qa, t3, ta, S3, SA, p.gap_open, p.gap_ext)
            bt_ref.check_valid(f[14], q3, qa, t3, ta, S3, SA, p.gap_open, p.gap_ext, alen, idn, gaps, want[4])
            assert (alen, idn, gaps, f[14]) == want[:4], (qk, t)
            n += 1
    return n


def test_search_with_backtraces_and_convertalis(O, dbs, monkeypatch):
    import unicore_amd as U
    d = dbs["dir"]
    opts = "-c 0.5 -e 10"
    U.search(dbs["qdb"], dbs["tdb"], d + "/plain_aln", d + "/tmp", opts)
    U.search(dbs["qdb"], dbs["tdb"], d + "/plain2_aln", d + "/tmp", opts + " -a 0")
    assert open(d + "/plain_aln", "rb").read() == open(d + "/plain2_aln", "rb").read()
    plain = _read_aln_db(d + "/plain_aln")
    assert all(len(f) == 14 for rr in plain.values() for f in rr)
    U.search(dbs["qdb"], dbs["tdb"], d + "/bt_aln", d + "/tmp", opts + " -a")
    rows = _read_aln_db(d + "/bt_aln")
    assert {k: [f[:14] for f in rr] for k, rr in rows.items()} == plain                 # -a adds a field and changes nothing else
    n = _check_rows(O, dbs, rows, "-c 0.5 -e 10")
    assert n >= 200
    assert any(len(dbs["s3q"][k]) > 2048 and rr for k, rr in rows.items())              # the long-query route served a row
    # small matrix budget and other bands: several batches, same strings
    for env in ({"UC_TB_BUDGET_MB": "1"}, {"UC_TB_BAND": "0"}, {"UC_TB_BAND": "4", "UC_TB_BUDGET_MB": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        U.search(dbs["qdb"], dbs["tdb"], d + "/bt2_aln", d + "/tmp", opts + " -a")
        assert open(d + "/bt2_aln", "rb").read() == open(d + "/bt_aln", "rb").read(), env
        for k in env:
            monkeypatch.delenv(k)
    # the all-int32 configuration through the engine
    U.search(dbs["qdb"], dbs["tdb"], d + "/bt3_aln", d + "/tmp", opts + " -a --sw-kernel i32")
    assert open(d + "/bt3_aln", "rb").read() == open(d + "/bt_aln", "rb").read()
    # convertalis
    U.convertalis(dbs["qdb"], dbs["tdb"], d + "/bt_aln", d + "/bt.m8")
    U.convertalis(dbs["qdb"], dbs["tdb"], d + "/plain_aln", d + "/plain.m8")
    assert open(d + "/bt.m8").read() == open(d + "/plain.m8").read()
    U.convertalis(dbs["qdb"], dbs["tdb"], d + "/bt_aln", d + "/bt.tsv", format_output="query,target,cigar,qaln,taln,qstart,qend,tstart,tend")
    let = np.frombuffer((util.LET + "X").encode(), np.uint8)
    k = 0
    for line in open(d + "/bt.tsv"):
        qn, tn, cigar, qaln, taln, qs, qe, ts, te = line.rstrip("\n").split("\t")
        aq = let[dbs["saq"][int(qn[1:])]].tobytes().decode(); at = let[dbs["sat"][int(tn[1:])]].tobytes().decode()
        assert qaln.replace("-", "") == aq[int(qs) - 1:int(qe)] and taln.replace("-", "") == at[int(ts) - 1:int(te)]
        assert len(qaln) == len(taln) == sum(n for n, _ in bt_ref.parse(cigar))
        k += 1
    assert k == n
    with pytest.raises(U.UcError):
        U.convertalis(dbs["qdb"], dbs["tdb"], d + "/plain_aln", d + "/x.tsv", format_output="query,cigar")


def test_cli_search_and_cluster_accept_the_flag(dbs):
    d = dbs["dir"]
    uni = os.path.join(util.ROOT, "bin", "unicore")
    env = dict(os.environ, UC_ALLOW_SYNTHETIC="1")
    for tag, so in (("a", "-c 0.5 -a"), ("b", "-c 0.5")):
        subprocess.check_call([uni, "search", "--keep-aln-db", "-s", so, dbs["tdb"], dbs["qdb"], d + "/cli_" + tag, d + "/tmp"], env=env,
                              stdout=subprocess.DEVNULL)
    assert open(d + "/cli_a.m8").read() == open(d + "/cli_b.m8").read() != ""
    assert all(len(f) == 15 for rr in _read_aln_db(d + "/cli_a_aln").values() for f in rr)
    assert all(len(f) == 14 for rr in _read_aln_db(d + "/cli_b_aln").values() for f in rr)
    import unicore_amd as U
    for tag, co in (("a", "-c 0.8 -a"), ("b", "-c 0.8")):
        U.cluster(dbs["qdb"], d + "/clu_" + tag, d + "/tmp", co)
        U.createtsv(dbs["qdb"], d + "/clu_" + tag, d + "/clu_" + tag + ".tsv")
    assert open(d + "/clu_a.tsv").read() == open(d + "/clu_b.tsv").read() != ""


def test_staged_api_mutual_hits(O):
    """all-vs-all on one database: (t, q) shares the traceback of (q, t) unless the walk met a gap-direction tie"""
    import unicore_amd as U
    s3, sa = util.family_db(8, n_fam=10, members=5, extra=(500,))
    p = util.oracle_params(O, "-c 0.5")
    S3, SA = bt_ref.matrices(p)
    got = {}
    for opts in ("-c 0.5 -a", "-c 0.5 -a --sym-dedup 0"):
        e = _engine(opts, s3, sa)
        e.prefilter(); e.align()
        cnt, hits = e.hits()
        al = e.alns()
        off, runs = e.backtraces()
        cig, k = {}, 0
        for q in range(e.n):
            for _ in range(int(cnt[q])):
                a, t = al[k], int(hits["target"][k])
                sl = runs[int(off[k]):int(off[k + 1])]
                if a["accepted"]:
                    cig[(q, t)] = (U.render_backtrace(sl), a)
                else:
                    assert len(sl) == 0
                k += 1
        got[opts] = cig
    first, second = got.values()
    assert {k: v[0] for k, v in first.items()} == {k: v[0] for k, v in second.items()} and len(first) >= 100
    mutual = swapped = 0
    for (q, t), (c, a) in first.items():
        qs, qe, ts, te = int(a["qstart"]), int(a["qend"]), int(a["tstart"]), int(a["tend"])
        q3, qa, t3, ta = s3[q][qs:qe + 1], sa[q][qs:qe + 1], s3[t][ts:te + 1], sa[t][ts:te + 1]
        want = bt_ref.traceback(q3, qa, t3, ta, S3, SA, p.gap_open, p.gap_ext)
        bt_ref.check_valid(c, q3, qa, t3, ta, S3, SA, p.gap_open, p.gap_ext, int(a["aln_len"]), int(a["idents"]), int(a["gap_opens"]), int(a["score"]))
        assert c == want[3], (q, t)                                   # every hit equals its own restatement ...
        if q != t and (t, q) in first:
            mutual += 1
            swapped += first[(t, q)][0] == bt_ref.swap_id(c)          # ... which for mutual hits is the partner's with I / D exchanged, ties apart
    assert mutual >= 20 and swapped >= mutual // 2
