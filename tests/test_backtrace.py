"""Alignment backtraces (-a), the part that needs no GPU: the tests' own restatement of the oracle's traceback (tests/bt_ref.py) is checked
against the oracle and against the validity list of a backtrace; the option table, the run renderer, --format-output parsing and
convertalis on hand-written alignment DBs."""
import os

import numpy as np
import pytest

import bt_ref
import util

EXTREME = "--mat-bit-factor-3di 9.5 --mat-bit-factor-aa 8.7 --gap-open 31 --gap-extend 3"      # matrices out to +-48, the largest gap open


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.mark.parametrize("opts", ["", EXTREME])
def test_restatement_matches_oracle_and_validity_list(O, opts):
    p = util.oracle_params(O, opts)
    S3, SA = bt_ref.matrices(p)
    rng = np.random.default_rng(11 + len(opts))
    s3, sa, pairs = bt_ref.pair_set(rng, [1, 2, 7, 33, 64, 90, 141, 160, 200, 257, 300], per_length=6)
    odb = O.OracleDb(s3=s3, sa=sa)
    n, kinds, gapped = 0, set(), 0
    for q, t, kind in pairs:
        b = bt_ref.box_of(O, p, s3[q], sa[q], s3[t], sa[t])
        boxes = [] if b is None else [b]
        same = np.nonzero(S3[s3[q][0], s3[t]] + SA[sa[q][0], sa[t]] > 0)[0]
        if len(same):                                                  # a one-residue box with a positive score
            j = int(same[0])
            boxes.append((int(S3[s3[q][0], s3[t][j]] + SA[sa[q][0], sa[t][j]]), 0, 0, j, j))
        for score, qs, qe, ts, te in boxes:
            q3, qa, t3, ta = s3[q][qs:qe + 1], sa[q][qs:qe + 1], s3[t][ts:te + 1], sa[t][ts:te + 1]
            ln, idn, gaps, cigar, h_end = bt_ref.traceback(q3, qa, t3, ta, S3, SA, p.gap_open, p.gap_ext)
            assert (ln, idn, gaps) == O.traceback(odb, p, q, t, qs, qe, ts, te), (q, t, kind)
            assert h_end == score == O.sw(q3, qa, t3, ta, p)[0]
            bt_ref.check_valid(cigar, q3, qa, t3, ta, S3, SA, p.gap_open, p.gap_ext, ln, idn, gaps, score)
            n += 1; kinds.add(kind); gapped += gaps > 0
    assert n >= 300 and kinds == {"mutated", "zigzag", "unrelated"} and gapped >= 50


def test_option_table_knows_the_backtrace_flags():
    import unicore_amd as U
    L = U.lib()
    assert L.uc_option_arity(b"-a") == 2
    assert L.uc_option_arity(b"--format-output") == 1
    for o in (b"-a", b"-a 1", b"-a 0", b"-c 0.8 -a", b"-a -c 0.8", b"-c 0.8 --format-output query,target,cigar"):
        assert L.uc_check_options(o) == 0, (o, U.last_error() if hasattr(U, "last_error") else "")
    assert L.uc_check_options(b"-a 2") != 0                         # "2" is no switch value and no flag


def test_run_renderer():
    import unicore_amd as U
    w = lambda n, op: (n << 2) | "MID".index(op)                    # noqa: E731
    assert U.render_backtrace([w(35, "M"), w(2, "D"), w(110, "M"), w(1, "I"), w(7, "M")]) == "35M2D110M1I7M"
    assert U.render_backtrace([]) == ""
    assert U.render_backtrace([w(65535, "M")]) == "65535M"
    with pytest.raises(U.UcError):
        U.render_backtrace([(5 << 2) | 3])                          # no such operation
    with pytest.raises(U.UcError):
        U.render_backtrace([0])                                     # a run of length 0


def test_format_output_parsing():
    import unicore_amd as U
    every = "query,target,fident,pident,nident,alnlen,mismatch,gapopen,qstart,qend,qlen,tstart,tend,tlen,evalue,bits,qcov,tcov,cigar,qaln,taln,qseq,tseq"
    assert U.format_output_columns(every) == 23
    assert U.format_output_columns("") == 12
    assert U.format_output_columns("cigar") == 1
    for bad in ("query,,target", "query,nosuch", "cigar,", "Query"):
        with pytest.raises(U.UcError):
            U.format_output_columns(bad)


# ---- convertalis on hand-written alignment DBs ----------------------------------------------------------------------------
Q_AA = "MKTAYIAKQRQISFVKSHFSRQ"
T_AA = "AYIAKQRWWISFVKSH"
# q[3..15] = AYIAKQR QISFVK  vs  t[0..13] = AYIAKQR WW ISFVK: 7M, 2 target-only residues, then q's Q alone, 5M
ROW14 = "1\t57\t0.800\t1.250E-09\t3\t15\t22\t0\t13\t16\t15\t12\t2\t61"
CIGAR = "7M2D1I5M"


def _write_dbs(tmp_path, row):
    def code(s):
        return np.array([util.LET.index(c) for c in s], np.uint8)
    db = str(tmp_path / "db")
    util.write_db(db, [code(Q_AA), code(T_AA)], [code(Q_AA), code(T_AA)], names=["qprot", "tprot"])
    aln = str(tmp_path / "res_aln")
    data = (row + "\n").encode() + b"\0"
    open(aln, "wb").write(data + b"\0")
    open(aln + ".index", "w").write("0\t0\t%d\n1\t%d\t1\n" % (len(data), len(data)))
    open(aln + ".dbtype", "wb").write((5).to_bytes(4, "little"))
    return db, aln


def test_convertalis_columns_from_a_15_field_db(tmp_path):
    import unicore_amd as U
    db, aln = _write_dbs(tmp_path, ROW14 + "\t" + CIGAR)
    out = str(tmp_path / "o.tsv")
    U.convertalis(db, db, aln, out, format_output="query,target,cigar,qaln,taln,qstart,qend,tstart,tend,qlen,tlen,nident,pident,qcov,qseq,tseq")
    f = open(out).read().rstrip("\n").split("\t")
    assert f[:3] == ["qprot", "tprot", CIGAR]
    assert f[3] == "AYIAKQR--QISFVK" and f[4] == "AYIAKQRWW-ISFVK"
    assert f[3].replace("-", "") == Q_AA[3:16] and f[4].replace("-", "") == T_AA[0:14]
    assert f[5:16] == ["4", "16", "1", "14", "22", "16", "12", "80.0", "0.591", Q_AA, T_AA]
    U.convertalis(db, db, aln, out)                                  # a 15-field DB through the default list: the 12 columns
    assert open(out).read() == "qprot\ttprot\t0.800\t15\t0\t2\t4\t16\t1\t14\t1.250E-09\t57\n"
    with pytest.raises(U.UcError):
        U.convertalis(db, db, aln, out, format_output="query,target,nosuchcolumn")


def test_convertalis_14_field_db(tmp_path):
    import unicore_amd as U
    db, aln = _write_dbs(tmp_path, ROW14)
    out = str(tmp_path / "o.m8")
    U.convertalis(db, db, aln, out)
    want = open(os.path.join(util.ROOT, "tests", "golden", "backtrace_default_columns.m8")).read()
    assert open(out).read() == want
    U.convertalis(db, db, aln, out, format_output="query,target,alnlen,bits")
    assert open(out).read() == "qprot\ttprot\t15\t57\n"
    for col in ("cigar", "qaln", "taln"):
        with pytest.raises(U.UcError) as ei:
            U.convertalis(db, db, aln, out, format_output="query," + col)
        assert "-a" in str(ei.value)
