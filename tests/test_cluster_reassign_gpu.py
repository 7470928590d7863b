"""Rule UC-1/R (--cluster-reassign) on the GPU: the stage's entry point (uc_engine_reassign: list, verdict, seed and map kernels of
uc_reassign.hip around the gapped stage and the prefilter) against the Python restatement of the rule (cluster_reassign_ref.py) on real and on
adversarial assignments, then the flag through every caller - uc_cluster on one and several (virtual) ranks, both CLIs, the plain step and the
exhaustive prefilter."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cluster_reassign_ref as R
import util

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
SHIM = os.path.join(util.ROOT, "bin", "foldseek")
EXE = os.path.join(util.ROOT, "bin", "unicore")
FIXTURE_OPTS = "-c 0.8 --min-seq-id 0.3 -s 7.5 --cluster-reassign"
FAMILY_OPTS = "-c 0.9 -e 1e-5"


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


@pytest.fixture(scope="module")
def family(O, tmp_path_factory):
    """the 100-sequence family database of the issue's table (seed 1; its last four sequences have length 1, 5, 9 and 15 x X), in memory and on disk"""
    s3, sa = util.family_db(1, n_fam=12, members=8, sub3=0.25, suba=0.4, indel=0.04)
    d = str(tmp_path_factory.mktemp("reassign"))
    names = util.write_db(os.path.join(d, "db"), s3, sa)
    return dict(s3=s3, sa=sa, odb=O.OracleDb(s3=s3, sa=sa), flat=util.flat(s3, sa), dir=d, prefix=os.path.join(d, "db"), names=names)


@pytest.fixture(scope="module")
def ref(O, U):
    """reference results, each computed once per session: ref(odb, opts, A=None) -> (A, result); A = None: the oracle workflow's assignment"""
    @functools.lru_cache(maxsize=None)
    def cached(odb_id, opts, key):
        odb, A = keep[odb_id], keep[key] if key is not None else None
        base, sw = R.split_options(opts)
        p = util.oracle_params(O, base)
        if A is None:
            A = R.workflow_assign(O, odb, p, sw)
        return A, R.reassign(O, U, odb, p, A, sw["cluster_mode"], sw["prefilter_mode"])
    keep = {}

    def get(odb, opts, A=None):
        keep[id(odb)] = odb
        key = None
        if A is not None:
            key = ("A", np.asarray(A, np.uint32).tobytes())
            keep[key] = np.asarray(A, np.uint32)
        return cached(id(odb), opts, key)
    return get


def engine_reassign(U, fam, opts, A):
    e = U.Engine(opts, verbosity=1)
    e.set_db(*fam["flat"])
    try:
        out = e.reassign(A)
        st = e.stats()
        # the engine is left with the full database and usable: the stage can run again and gives the same answer
        assert e.n == len(fam["s3"])
        again = e.reassign(A)
        assert np.array_equal(again[0], out[0]) and np.array_equal(again[1], out[1]) and again[2] == out[2]
    finally:
        e.close()
    return out + (st,)


def check_against(res, got):
    a, rej, cnt, st = got
    print("counts (verified, rejected, re-search pairs, clusters): device", tuple(cnt.values()), "reference", res["counts"])
    assert np.array_equal(rej, res["rejected"])
    assert tuple(cnt.values()) == res["counts"]
    assert np.array_equal(a, res["assign"])
    assert st["n_gapped_alignments"] >= res["counts"][0]


@pytest.mark.parametrize("rule", ["", " --cluster-mode 2 --cov-mode 1"])
def test_entry_point_on_the_workflow_assignment(U, family, ref, rule):
    """Engine.reassign fed the oracle workflow's assignment: rejected flags, counts and final assignment are the reference's, under both rules"""
    A, res = ref(family["odb"], FAMILY_OPTS + rule)
    if not rule:
        assert res["counts"][:2] == (63, 4)
    assert res["counts"][1] > 0
    check_against(res, engine_reassign(U, family, FAMILY_OPTS + rule, A))


def test_one_list_longer_than_max_seqs(U, family, ref):
    """everything assigned to sequence 0: one list of 99 members under --max-seqs 20, most of them rejected, a re-search with 95+ queries"""
    n = len(family["s3"])
    A = np.zeros(n, np.uint32)
    opts = FAMILY_OPTS + " --max-seqs 20"
    _, res = ref(family["odb"], opts, A)
    assert res["counts"][0] == n - 1 and res["counts"][1] > n // 2
    check_against(res, engine_reassign(U, family, opts, A))


def test_identity_assignment(U, family, ref):
    """no members: empty lists, no verification, step 3 skipped, every sequence its own cluster"""
    n = len(family["s3"])
    A = np.arange(n, dtype=np.uint32)
    _, res = ref(family["odb"], FAMILY_OPTS, A)
    assert res["counts"] == (0, 0, 0, n)
    got = engine_reassign(U, family, FAMILY_OPTS, A)
    check_against(res, got)
    assert got[3]["n_gapped_alignments"] == 0


def test_rejected_sequences_without_a_kmer(U, family, ref):
    """the sequences of length 1, 5, 9 and the all-X one are put into the first cluster of the workflow's assignment: they are rejected, have no
    k-mer hit in the re-search and come out as singletons"""
    A0, _ = ref(family["odb"], FAMILY_OPTS)
    n = len(A0)
    A = np.array(A0, np.uint32)
    A[n - 4:] = A[0]
    _, res = ref(family["odb"], FAMILY_OPTS, A)
    assert res["rejected"][n - 4:].all()
    assert res["assign"][n - 4:].tolist() == list(range(n - 4, n))
    check_against(res, engine_reassign(U, family, FAMILY_OPTS, A))


def test_malformed_assignments_are_refused(U, family):
    n = len(family["s3"])
    e = U.Engine(FAMILY_OPTS, verbosity=1)
    e.set_db(*family["flat"])
    chain = np.arange(n, dtype=np.uint32)
    chain[1], chain[2] = 2, 3                       # 1 -> 2 -> 3: not idempotent
    out_of_range = np.arange(n, dtype=np.uint32)
    out_of_range[n - 1] = n
    for bad in (chain, out_of_range):
        with pytest.raises(U.UcError) as ei:
            e.reassign(bad)
        assert ei.value.code == U.UC_ERR_ARGS
    a, rej, cnt = e.reassign(np.arange(n, dtype=np.uint32))      # usable after the refusals
    assert cnt["clusters"] == n and not rej.any()
    e.close()


def _cluster_tsv(U, db, d, tag, opts, num_gpus=1):
    st = U.cluster(db, os.path.join(d, tag + "_cluster"), os.path.join(d, "tmp"), opts, threads=4, num_gpus=num_gpus)
    U.createtsv(db, os.path.join(d, tag + "_cluster"), os.path.join(d, tag + ".tsv"))
    return open(os.path.join(d, tag + ".tsv"), "rb").read(), st


def _ref_tsv(O, odb, assign, path):
    O.write_tsv(path, odb, assign)
    return open(path, "rb").read()


@pytest.fixture(scope="module")
def golden(O, U, ref, tmp_path_factory):
    """the golden database: the one-rank results of uc_cluster that several tests compare against"""
    d = str(tmp_path_factory.mktemp("reassign_golden"))
    db = os.path.join(GOLD, "db")
    out = dict(dir=d, db=db, odb=O.OracleDb(db))
    out["flag"], out["flag_st"] = _cluster_tsv(U, db, d, "flag", FIXTURE_OPTS)
    return out


def test_uc_cluster_writes_the_fixture(U, O, golden, ref, tmp_path):
    want = open(os.path.join(GOLD, "clust_reassign.tsv"), "rb").read()
    assert golden["flag"] == want
    A, res = ref(golden["odb"], FIXTURE_OPTS)
    st = golden["flag_st"]
    assert st["n_clusters"] == res["counts"][3] == 48
    d, db = golden["dir"], golden["db"]
    base = FIXTURE_OPTS.replace(" --cluster-reassign", "")
    plain, st0 = _cluster_tsv(U, db, d, "plain", base)
    off, st_off = _cluster_tsv(U, db, d, "off", base + " --cluster-reassign 0")
    assert off == plain and plain != want
    assert st_off["n_gapped_alignments"] == st0["n_gapped_alignments"]
    assert st["n_gapped_alignments"] >= st0["n_gapped_alignments"] + res["counts"][0]        # the stage's pairs are counted
    # nothing rejected under a bare -c 0.8: step 3 is skipped, step 4 still runs
    A1, res1 = ref(golden["odb"], "-c 0.8 --cluster-reassign")
    assert res1["counts"][1] == 0
    got1, st1 = _cluster_tsv(U, db, d, "bare", "-c 0.8 --cluster-reassign")
    assert got1 == _ref_tsv(O, golden["odb"], res1["assign"], str(tmp_path / "bare_ref.tsv"))
    assert st1["n_clusters"] == res1["counts"][3]


def test_both_clis(golden, tmp_path):
    db, want = golden["db"], golden["flag"]
    out = str(tmp_path / "u" / "clust")
    r = subprocess.run([EXE, "cluster", db, out, str(tmp_path / "tmp"), "-c", FIXTURE_OPTS, "--threads", "4"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert open(out + ".tsv", "rb").read() == want
    out = str(tmp_path / "f" / "clust")
    os.makedirs(os.path.dirname(out))
    for argv in ([SHIM, "cluster", "--cluster-reassign", "--threads", "4", "-v", "3", db, out + "_cluster", str(tmp_path / "ftmp")] + FIXTURE_OPTS.replace(" --cluster-reassign", "").split(),
                 [SHIM, "createtsv", "--threads", "4", "-v", "2", db, db, out + "_cluster", out + ".tsv"]):
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, (argv, r.stdout[-2000:], r.stderr[-2000:])
        if argv[1] == "cluster":      # the -v 3 line of the stage
            assert "reassign: 47 members verified, 4 rejected, 0 re-search pairs accepted, 44 -> 48 clusters" in r.stdout + r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    assert open(out + ".tsv", "rb").read() == want


@pytest.mark.parametrize("gpus,shards", [(2, ""), (4, " --target-shards 2")])
def test_several_ranks_write_the_same_file(U, golden, monkeypatch, gpus, shards):
    monkeypatch.setenv("UC_VIRTUAL_GPUS", "1")
    got, st = _cluster_tsv(U, golden["db"], golden["dir"], "g%d" % gpus, FIXTURE_OPTS + shards, num_gpus=gpus)
    assert st["n_gpus"] == gpus
    assert got == golden["flag"]
    assert st["n_clusters"] == golden["flag_st"]["n_clusters"]


def test_plain_step_with_the_flag(U, O, family, ref, tmp_path):
    """--single-step-clustering --cluster-reassign: the verify direction (representative as the query) can reject after a plain step too"""
    opts = FAMILY_OPTS + " --single-step-clustering --cluster-reassign"
    A, res = ref(family["odb"], opts)
    got, st = _cluster_tsv(U, family["prefix"], family["dir"], "single", opts)
    assert got == _ref_tsv(O, O.OracleDb(family["prefix"]), res["assign"], str(tmp_path / "ref.tsv"))
    assert st["n_clusters"] == res["counts"][3]
    util.tsv_invariants(os.path.join(family["dir"], "single.tsv"), family["names"])


def test_exhaustive_prefilter_with_the_flag(U, O, family, ref, tmp_path):
    """--prefilter-mode 1 --cluster-reassign: the stage's input is what the workflow writes under that mode without the flag (tested on its own in
    test_prefilter_mode1_gpu.py); the re-search of the reference scores every diagonal (ungapped_all_ref.py)"""
    opts = FAMILY_OPTS + " --prefilter-mode 1"
    plain, _ = _cluster_tsv(U, family["prefix"], family["dir"], "x_plain", opts)
    idx = {nm: i for i, nm in enumerate(family["names"])}
    A = np.zeros(len(idx), np.uint32)
    for line in plain.decode().splitlines():
        rep, mem = line.split("\t")
        A[idx[mem]] = idx[rep]
    _, res = ref(family["odb"], opts, A)
    assert res["counts"][1] > 0, "nothing rejected: the case tests nothing"
    got, st = _cluster_tsv(U, family["prefix"], family["dir"], "x_flag", opts + " --cluster-reassign")
    assert got == _ref_tsv(O, O.OracleDb(family["prefix"]), res["assign"], str(tmp_path / "ref.tsv"))
    assert st["n_clusters"] == res["counts"][3]
