"""Kernel-level parity of the linear-time pre-step (uc_linclust.hip, spec UC-1 E8a) on X, repeats, duplicates and ties: Engine.linclust_pairs
(uc_engine_linclust_pairs) against the oracle and against the plain-Python restatement of tests/linclust_ref.py on every (case, m, pattern) of
the shared case list - exact integer comparisons, no tolerance anywhere.  That the list reaches the branches it was built for is proven on the
CPU in tests/test_linclust_cases.py.  Then the whole pre-step round of uc_cluster on the combined edge database: on one rank (the pairs become the
hit lists on the device) and on 2 and 3 virtual ranks (the pairs go through the host and are dealt out by centre mod world).

That these tests can fail was checked with three value-only mutations of uc_linclust.hip on a scratch copy (never committed), each run once:
  lc_select_kernel skipping equal hashes (`above` without its position clause) -> the pair tests of all three patterns, install mode, reuse and both
      one-rank rounds red; first seen at ("repeats", m = 5): the extra pair (6, 7) with the one-k-mer partner that holds the (m + 1)-th pick;
  lc_group_kernel choosing the centre with `ls >= lc` (ties to the LARGEST id) -> the same tests and the m override / bad-argument tests red; first
      seen at ("x", m = 1): (3, 2) instead of (2, 3) for the sequence and its equally long copy with an X under a `0`;
  the pair sort over pbits - 1 bits -> the pair, install, reuse, override and bad-argument tests and the m = 5 one-rank round red; first seen at
      ("lengths", m = 1), ("centre", 20) and ("n3", 20): the pairs of the centres with the top bit of the key set come out in front
      ([[2, 0], [2, 1], [1, 0]] for n = 3).
The virtual-rank tests compare a build with itself and stay green under all three; the one-rank round is what ties them to the oracle.
The whole module takes 4.0 s on an MI355X, oracle and restatement included."""
import os

import numpy as np
import pytest

import linclust_ref as LR
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    return unicore_amd


@pytest.fixture(scope="module")
def engines(U):
    """one engine per spaced pattern: the m override serves every m"""
    es = {pat: U.Engine("-c 0.8 --spaced-kmer-pattern " + pat, verbosity=1) for pat in LR.PATTERNS}
    yield es
    for e in es.values():
        e.close()


def _set_db(e, s3):
    off, c3, _ = util.flat(s3, s3)
    e.set_db(off, c3, np.zeros(len(c3), np.uint8))


def _same(got, ref, what):
    assert got.shape == ref.shape and np.array_equal(got, ref), (what, len(got), len(ref), got[:6].tolist(), ref[:6].tolist())


@pytest.mark.parametrize("pattern", LR.PATTERNS, ids=LR.PATTERN_IDS)
def test_pairs_equal_oracle_and_restatement(O, engines, pattern):
    e, ref = engines[pattern], LR.reference(pattern)
    for name, s3, ms in LR.cases(pattern):
        _set_db(e, s3)
        for m in ms:
            got = e.linclust_pairs(m)
            _same(got, ref[(name, m)][0], (name, m, "restatement"))
            _same(got, LR.oracle_pairs(O, s3, pattern, m), (name, m, "oracle"))


@pytest.mark.parametrize("pattern", LR.PATTERNS, ids=LR.PATTERN_IDS)
def test_install_mode_lists_are_the_pairs(engines, pattern):
    """install = 1: the returned count, hits() (targets in order, score 0, diag 0, per-centre counts) and the pair list agree - also where there is
    no entry or no pair at all (empty lists, zero counts)"""
    e, ref = engines[pattern], LR.reference(pattern)
    for name, s3, ms in LR.cases(pattern):
        _set_db(e, s3)
        for m in [x for x in ms if x != 1000]:
            pr = ref[(name, m)][0]
            assert e.linclust_pairs(m, install=True) == len(pr) == e.hits_size(), (name, m)
            cnt, hits = e.hits()
            assert np.array_equal(cnt, np.bincount(pr[:, 0], minlength=len(s3)).astype(np.uint32)), (name, m)
            assert np.array_equal(hits["target"], pr[:, 1]) and not hits["score"].any() and not hits["diag"].any(), (name, m)
            _same(e.linclust_pairs(m), pr, (name, m, "pair list after install"))


def test_scratch_reuse_leaves_nothing_behind(engines):
    """a second call on the same engine, a call after set_db with a smaller and a larger case, the engine's own --kmer-per-seq (m = None): nothing
    of the previous database or m may be left in the reused buffers"""
    pat = LR.PATTERNS[0]
    e, ref = engines[pat], LR.reference(pat)
    by = {c[0]: c[1] for c in LR.cases(pat)}
    for name, m in (("big", 300), ("big", 300), ("n3", 20), ("no_valid", 300), ("centre", 5), ("big", 20), ("n1", 1), ("overlap", 300), ("combined", 20), ("x", 1)):
        _set_db(e, by[name])
        _same(e.linclust_pairs(m), ref[(name, m)][0], (name, m))
        _same(e.linclust_pairs(m), ref[(name, m)][0], (name, m, "again"))
    _set_db(e, by["big"])
    assert e.linclust_pairs(20, install=True) == len(ref[("big", 20)][0])
    _set_db(e, by["no_valid"])
    assert e.linclust_pairs(20, install=True) == 0 and e.hits_size() == 0 and not e.hits()[0].any()
    _set_db(e, by["centre"])
    _same(e.linclust_pairs(), ref[("centre", 20)][0], "m = None is --kmer-per-seq 20")


def test_engine_kmer_per_seq_is_the_default_m(U):
    pat = LR.PATTERNS[0]
    e = U.Engine("-c 0.8 --kmer-per-seq 5", verbosity=1)
    try:
        _set_db(e, LR.centre_case(pat))
        _same(e.linclust_pairs(), LR.reference(pat)[("centre", 5)][0], "m = None")
        _same(e.linclust_pairs(300), LR.reference(pat)[("centre", 300)][0], "override")
    finally:
        e.close()


def test_bad_arguments_are_refused(U, engines):
    e = engines[LR.PATTERNS[0]]
    _set_db(e, LR.centre_case(LR.PATTERNS[0]))
    for m in (1001, 65536, 0, -1):
        with pytest.raises(U.UcError) as err:
            e.linclust_pairs(m)
        assert err.value.code == U.UC_ERR_ARGS, m
    L = U.lib()
    import ctypes as C
    n = C.c_uint64()
    assert L.uc_engine_linclust_pairs(e._h, 1001, 0, None, 0, C.byref(n)) == U.UC_ERR_ARGS
    assert L.uc_engine_linclust_pairs(e._h, 20, 2, None, 0, C.byref(n)) == U.UC_ERR_ARGS
    assert L.uc_engine_linclust_pairs(e._h, 20, 0, None, 0, None) == U.UC_ERR_ARGS
    assert L.uc_engine_linclust_pairs(None, 20, 0, None, 0, C.byref(n)) == U.UC_ERR_ARGS
    assert L.uc_engine_linclust_pairs(e._h, 20, 0, None, 8, C.byref(n)) == U.UC_ERR_ARGS          # room announced, no buffer
    assert L.uc_engine_linclust_pairs(e._h, 0, 0, None, 0, C.byref(n)) == 0 and n.value == len(LR.reference(LR.PATTERNS[0])[("centre", 20)][0])   # count only
    fresh = U.Engine("-c 0.8", verbosity=1)
    try:
        with pytest.raises(U.UcError) as err:
            fresh.linclust_pairs(5)                   # no database
        assert err.value.code == U.UC_ERR_ARGS
    finally:
        fresh.close()
    _same(e.linclust_pairs(20), LR.reference(LR.PATTERNS[0])[("centre", 20)][0], "the engine is still usable")


# ---------------------------------------------------------------- the whole pre-step round of uc_cluster
ALN_ALWAYS = ("score", "score_rev", "corrected", "pass_evalue", "accepted")
ALN_IF_PASSED = ("qstart", "qend", "tstart", "tend")
ROUND_OPTS = (("-c 0.8 --linclust 1 --cluster-steps 1", 20), ("-c 0.8 --linclust 1 --cluster-steps 1 --kmer-per-seq 5", 5))


@pytest.fixture(scope="module")
def edge_db(tmp_path_factory):
    """the combined edge database (without the 65,535-residue sequence) on disk -> (prefix, s3, names)"""
    s3 = LR.combined(LR.PATTERNS[0])
    prefix = str(tmp_path_factory.mktemp("lc_edge") / "db")
    names = util.write_db(prefix, s3, [np.zeros(len(x), np.uint8) for x in s3])
    return prefix, s3, names


_ONE_RANK = {}


def _cluster(U, db, out, opts, num_gpus=1, env=None, hook=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    U.set_round_hook(hook)
    try:
        st = U.cluster(db, out + "_cluster", out + "_tmp", opts, threads=4, num_gpus=num_gpus)
    finally:
        U.set_round_hook(None)
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    U.createtsv(db, out + "_cluster", out + ".tsv")
    with open(out + ".tsv", "rb") as f:
        return f.read(), st


def _one_rank(U, edge_db, tmp, opts):
    """uc_cluster on one rank with the observer taking ALL of round -1: hit lists, alignment records, the round's n_prefilter_hits; once per session"""
    if opts not in _ONE_RANK:
        seen, errors = {}, []

        def hook(rnd, ids, kthr, view):
            try:
                if rnd == -1:
                    cnt, hits = view.hits_range(0, len(ids))
                    seen.update(ids=ids, cnt=cnt.copy(), hits=hits.copy(), alns=view.alns_range(0, len(ids)).copy(), n_pairs=view.hits_size(),
                                n_prefilter_hits=view.stats()["n_prefilter_hits"])
                seen.setdefault("rounds", []).append(rnd)
            except Exception as ex:          # an exception cannot cross the C frame
                errors.append(ex)
        tsv, st = _cluster(U, edge_db[0], str(tmp / ("one_%d" % len(_ONE_RANK))), opts, hook=hook)
        if errors:
            raise errors[0]
        _ONE_RANK[opts] = (tsv, st, seen)
    return _ONE_RANK[opts]


@pytest.mark.parametrize("opts,m", ROUND_OPTS, ids=["m20", "m5"])
def test_pre_step_round_on_one_rank(O, U, edge_db, tmp_path_factory, opts, m):
    prefix, s3, names = edge_db
    tsv, st, seen = _one_rank(U, edge_db, tmp_path_factory.mktemp("lc_one"), opts)
    odb = O.OracleDb(prefix)
    p = util.oracle_params(O, "-c 0.8")
    ref = O.cluster_workflow(odb, p, O.cascade_thresholds(p, 4.0, 1), linclust_m=m, threads=8)
    ref_tsv = str(tmp_path_factory.mktemp("lc_ref") / "ref.tsv")
    O.write_tsv(ref_tsv, odb, ref["assign"])
    with open(ref_tsv, "rb") as f:
        assert tsv == f.read()
    out_tsv = str(tmp_path_factory.mktemp("lc_tsv") / "clust.tsv")
    with open(out_tsv, "wb") as f:
        f.write(tsv)
    util.tsv_invariants(out_tsv, names)
    assert st["n_clusters"] == ref["counts"]["n_clusters"] and st["n_gapped_alignments"] == ref["counts"]["n_alignments"]
    # round -1: the hit lists are the pair list, all of it
    pr = np.asarray(O.linclust_pairs(odb, p, m), np.uint32).reshape(-1, 2)
    _same(pr, LR.reference(LR.PATTERNS[0])[("combined", m)][0], "oracle on the files == restatement on the arrays")
    assert seen["rounds"] == [-1, 0] and np.array_equal(seen["ids"], np.arange(len(s3)))
    assert seen["n_pairs"] == seen["n_prefilter_hits"] == len(pr) > 900
    assert np.array_equal(seen["cnt"], np.bincount(pr[:, 0], minlength=len(s3)).astype(np.uint32))
    hits, al = seen["hits"], seen["alns"]
    assert np.array_equal(hits["target"], pr[:, 1]) and not hits["score"].any() and not hits["diag"].any()
    # the alignment record of every pair, the centre as query
    assert len(al) == len(pr)
    ms = {int(c): O.min_score(odb, p, int(c)) for c in np.unique(pr[:, 0])}
    memo = {}
    for k, (c, t) in enumerate(pr.tolist()):
        key = (s3[c].tobytes(), s3[t].tobytes())          # 300 exact copies: one oracle alignment per distinct (centre, member) content
        if key not in memo:
            memo[key] = O.align_pair(odb, p, c, t, ms[c])
        r = memo[key]
        for f in ALN_ALWAYS:
            assert int(al[f][k]) == int(r[f]), (c, t, f, int(al[f][k]), int(r[f]))
        if r["pass_evalue"] == 1:
            for f in ALN_IF_PASSED:
                assert int(al[f][k]) == int(r[f]), (c, t, f, int(al[f][k]), int(r[f]))


@pytest.mark.parametrize("opts,m", ROUND_OPTS, ids=["m20", "m5"])
@pytest.mark.parametrize("ranks", [2, 3])
def test_pre_step_round_on_virtual_ranks(U, edge_db, tmp_path_factory, opts, m, ranks):
    """the pairs through the host, dealt out by centre mod world into set_hits: the one-rank TSV byte for byte, the same number of gapped alignments"""
    tsv1, st1, _ = _one_rank(U, edge_db, tmp_path_factory.mktemp("lc_one"), opts)
    tsv, st = _cluster(U, edge_db[0], str(tmp_path_factory.mktemp("lc_v") / "v"), opts, num_gpus=ranks, env={"UC_VIRTUAL_GPUS": "1"})
    assert tsv == tsv1
    assert st["n_gapped_alignments"] == st1["n_gapped_alignments"] and st["n_clusters"] == st1["n_clusters"]
