"""Rule UC-1/R (--cluster-reassign) without a GPU: the option parser, the Python restatement of the rule (cluster_reassign_ref.py) on the
databases where the transitive merge of the workflow is known to leave unverified members, the rule's consequence, and the committed fixture
tests/golden/clust_reassign.tsv."""
import os
import sys

import numpy as np
import pytest

import cluster_reassign_ref as R
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
FIXTURE_OPTS = "-c 0.8 --min-seq-id 0.3 -s 7.5 --cluster-reassign"


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.fixture(scope="module")
def G():
    sys.path.insert(0, GOLD)
    try:
        import make_clust_reassign
    finally:
        sys.path.remove(GOLD)
    return make_clust_reassign


@pytest.fixture(scope="module")
def golden(O, G):
    """the golden database under the fixture's options and under a bare -c 0.8: (odb, {opts: (A, result)}), computed once"""
    odb = O.OracleDb(os.path.join(GOLD, "db"))
    return odb, {opts: G.reference(odb, opts) for opts in (FIXTURE_OPTS, "-c 0.8 --cluster-reassign")}


def test_parser_accepts_the_switch(U):
    for ok in ("--cluster-reassign", "--cluster-reassign 1", "--cluster-reassign 0", "-c 0.8 --cluster-reassign", "--cluster-reassign -c 0.8",
               "--single-step-clustering --cluster-reassign", "--cluster-mode 2 --cluster-reassign 1 --prefilter-mode 1"):
        assert U.check_options(ok) == 0, (ok, U.lib().uc_last_error())
    assert U.lib().uc_option_arity(b"--cluster-reassign") == 2
    assert U.check_options("--cluster-reassign 2") == U.UC_ERR_ARGS      # 2 is no switch value and no flag


def test_refused_together_with_a_min_score_table(U, tmp_path):
    t = str(tmp_path / "ms.txt")
    open(t, "w").write("30 30 30\n")
    for bad in ("--single-step-clustering --min-score-table %s --cluster-reassign" % t, "--cluster-reassign 1 --single-step-clustering --min-score-table %s" % t):
        assert U.check_options(bad) == U.UC_ERR_ARGS, bad
        assert "min-score-table" in U.lib().uc_last_error().decode()
    assert U.check_options("--single-step-clustering --min-score-table %s --cluster-reassign 0" % t) == 0


def test_abi_and_binding(U):
    assert U.ABI_VERSION == 9 and U.lib().uc_abi_version() == 9
    assert "uc_engine_reassign" in U.SYMBOLS and hasattr(U.lib(), "uc_engine_reassign")
    hdr = open(os.path.join(util.ROOT, "include", "unicore_cluster.h")).read()
    assert "#define UC_ABI_VERSION 9" in hdr and "int uc_engine_reassign(" in hdr
    assert hasattr(U.Engine, "reassign")


def test_split_options():
    base, sw = R.split_options("-c 0.9 -e 1e-5 --cluster-mode 3 --cluster-reassign 1 --prefilter-mode 1 --single-step-clustering -s 6")
    assert base == "-c 0.9 -e 1e-5 -s 6"
    assert sw == dict(cluster_mode=2, prefilter_mode=1, single_step=True, reassign=True, sens=6.0)
    assert R.split_options("--cluster-reassign 0 -c 0.8")[1]["reassign"] is False


def test_reference_reproduces_the_rejections_on_the_golden_database(golden):
    odb, res = golden
    A, r = res[FIXTURE_OPTS]
    assert int((A != np.arange(odb.n)).sum()) == 47 and r["counts"][0] == 47
    assert r["counts"][1] == 4 and int(r["rejected"].sum()) == 4
    A0, r0 = res["-c 0.8 --cluster-reassign"]
    assert int((A0 != np.arange(odb.n)).sum()) == 50 and r0["counts"][:3] == (50, 0, 0)
    # nothing rejected: the graph is the star forest of A; the rule may only move representatives inside a cluster
    assert len(r0["edges"]) == 50 and r0["counts"][3] == int((A0 == np.arange(odb.n)).sum())
    same = lambda a, b: np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :])
    assert same(np.asarray(A0), np.asarray(r0["assign"]))


@pytest.mark.parametrize("seed,members,rejected", [(1, 63, 4), (2, 45, 2), (3, 50, 1)])
def test_reference_on_the_family_databases(O, U, seed, members, rejected):
    s3, sa = util.family_db(seed, n_fam=12, members=8, sub3=0.25, suba=0.4, indel=0.04)
    odb = O.OracleDb(s3=s3, sa=sa)
    base, sw = R.split_options("-c 0.9 -e 1e-5")
    p = util.oracle_params(O, base)
    A = R.workflow_assign(O, odb, p, sw)
    r = R.reassign(O, U, odb, p, A)
    assert r["counts"][:2] == (members, rejected)
    a = r["assign"]
    assert np.array_equal(a[a], a)
    assert R.unaccepted_members(O, odb, p, r) == []
    # before the rule the rejected members are exactly the ones without an accepted alignment from their representative
    assert [x for x in range(odb.n) if A[x] != x and not R.accepted(O, odb, p, int(A[x]), x)] == r["research"]


def test_every_member_is_accepted_by_its_representative_after_the_rule(O, golden):
    odb, res = golden
    for opts, (A, r) in res.items():
        p = util.oracle_params(O, R.split_options(opts)[0])
        a = r["assign"]
        assert np.array_equal(a[a], a), opts
        assert R.unaccepted_members(O, odb, p, r) == [], opts


def test_committed_fixture(O, golden, tmp_path):
    """tests/golden/clust_reassign.tsv: the generator still reproduces it, it satisfies the consumer's contract, and it is not what the workflow
    writes without the flag"""
    odb, res = golden
    A, r = res[FIXTURE_OPTS]
    want = open(os.path.join(GOLD, "clust_reassign.tsv"), "rb").read()
    O.write_tsv(str(tmp_path / "ref.tsv"), odb, r["assign"])
    assert open(tmp_path / "ref.tsv", "rb").read() == want
    names = [l.split("\t")[1] for l in open(os.path.join(GOLD, "db.lookup"))]
    util.tsv_invariants(os.path.join(GOLD, "clust_reassign.tsv"), names)
    O.write_tsv(str(tmp_path / "plain.tsv"), odb, A)
    assert open(tmp_path / "plain.tsv", "rb").read() != want, "the fixture equals the workflow's result without the flag: it tests nothing"
