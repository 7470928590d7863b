"""CPU preconditions of the custom-matrix and k-mer-pattern cases (tests/matrix_cases.py): what tests/test_custom_matrices_gpu.py and
tests/test_prefilter_matrices_gpu.py rely on, proven with the oracle and plain numpy only."""
import numpy as np
import pytest

import linclust_ref as LR
import matrix_cases as MC
import prefilter_cases as PC
import util
from sw_dp import Dp


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.fixture(scope="module")
def mats(O, tmp_path_factory):
    d = tmp_path_factory.mktemp("matrices")
    return {name: MC.write_case(O, name, d) for name in MC.NAMES}


def test_matrices_are_what_they_claim(O, mats):
    B3, BA = MC.base(O)
    assert (B3 == B3.T).all() and (BA == BA.T).all() and B3[:20, :20].max() <= 38       # what the suite had before: symmetric, small
    for name, (S3, SA, mo) in mats.items():
        assert S3.min() >= -48 and S3.max() <= 48 and SA.min() >= -48 and SA.max() <= 48, name
        p = util.oracle_params(O, "-c 0.8 " + mo)                                        # the files give the arrays back through the oracle's loader
        assert np.array_equal(np.array(p.S3[:], np.int32).reshape(21, 21), S3) and np.array_equal(np.array(p.SA[:], np.int32).reshape(21, 21), SA), name
        diag = int(np.trace(S3[:20, :20]))
        assert p.kmer_thr == int(np.floor(6 * diag / 20.0 + 3.0 - 8.0 + 0.5)), name      # derived from the LOADED diagonal
    sym = {name: ((S3 == S3.T).all(), (SA == SA.T).all()) for name, (S3, SA, _) in mats.items()}
    assert sym["directed"] == (False, False) and sym["perturbed"] == (False, False)
    assert sym["only_s3"] == (False, True) and sym["only_sa"] == (True, False)
    assert sym["hot"] == sym["mixed_hot"] == sym["negative"] == (True, True)
    assert np.array_equal(mats["only_s3"][1], BA) and np.array_equal(mats["only_sa"][0], B3)          # the other track untouched
    S3 = mats["perturbed"][0]
    assert (S3 != S3.T).sum() > 300                                                      # most of the 380 off-diagonal entries
    assert (np.diag(mats["hot"][0])[:20] == 48).all()
    assert mats["negative"][0][list(MC.NEG_LETTERS)][:, :20].max() <= -20


def test_directed_case(O, mats):
    """base -> copy scores the self score, copy -> base far lower; one-way prefilter hits; a mutual hit whose two directions differ"""
    S3, SA, mo = mats["directed"]
    opts = "-c 0.8 " + mo
    p = util.oracle_params(O, opts)
    s3, sa = MC.directed_db()
    assert len(s3) == 16 and all(60 <= len(x) <= 300 for x in s3)
    for i in range(0, len(s3), 2):
        own = int(S3[s3[i], s3[i]].sum() + SA[sa[i], sa[i]].sum())
        fwd = O.sw(s3[i], sa[i], s3[i + 1], sa[i + 1], p)
        back = O.sw(s3[i + 1], sa[i + 1], s3[i], sa[i], p)
        assert fwd == (own, len(s3[i]) - 1, len(s3[i]) - 1), i
        assert 0 < back[0] < own // 2, (i, back, own)
    ref = O.cluster(O.OracleDb(s3=s3, sa=sa), p, threads=4)
    cnt = ref["hit_cnt"]
    rec = {(q, int(h["t"])): ref["aln"][q, k] for q in range(len(cnt)) for k, h in enumerate(ref["hits"][q, : cnt[q]])}
    one_way = [k for k in rec if (k[1], k[0]) not in rec]
    mutual = [k for k in rec if k[0] < k[1] and (k[1], k[0]) in rec]
    assert one_way and mutual
    assert any(rec[q, t]["score"] != rec[t, q]["score"] for q, t in mutual)
    assert any(rec[q, t]["accepted"] != rec[t, q]["accepted"] for q, t in mutual)
    assert len(set(ref["assign"].tolist())) == 8                                        # the oracle clusters every family
    print("directed: %d hits, %d one-way, %d mutual" % (len(rec), len(one_way), len(mutual)))


def test_perturbed_case(O, mats):
    S3, SA, mo = mats["perturbed"]
    p = util.oracle_params(O, "-c 0.8 " + mo)
    s3, sa = MC.family_case_db()
    ref = O.cluster(O.OracleDb(s3=s3, sa=sa), p, threads=4)
    cnt = ref["hit_cnt"]
    rec = {(q, int(h["t"])): ref["aln"][q, k] for q in range(len(cnt)) for k, h in enumerate(ref["hits"][q, : cnt[q]])}
    mutual = [k for k in rec if k[0] < k[1] and (k[1], k[0]) in rec]
    differ = sum(1 for q, t in mutual if rec[q, t]["score"] != rec[t, q]["score"])
    verdicts = sum(1 for q, t in mutual if rec[q, t]["accepted"] != rec[t, q]["accepted"])
    print("perturbed: %d mutual hits, %d with different scores, %d with different verdicts" % (len(mutual), differ, verdicts))
    assert differ >= 20          # (opposite verdicts are the directed case's business)


@pytest.mark.parametrize("name", ["directed", "perturbed"])
def test_numpy_dp_equals_the_oracle_under_asymmetric_matrices(O, mats, name):
    """Dp indexes S[query letter][target letter] by numpy fancy indexing, the oracle by its own loop: both orientations of every pair"""
    p = util.oracle_params(O, "-c 0.8 " + mats[name][2])
    dp = Dp(p)
    s3, sa = MC.directed_db() if name == "directed" else MC.family_case_db()
    rng = np.random.default_rng(1)
    pairs = [(i, i ^ 1) for i in range(16)] + [tuple(x) for x in rng.integers(0, len(s3) - 4, (24, 2))]
    asym = 0
    for q, t in pairs:
        a = dp.summary(s3[q], sa[q], s3[t], sa[t])[0]
        assert a == tuple(O.sw(s3[q], sa[q], s3[t], sa[t], p)), (q, t)
        asym += a[0] != dp.summary(s3[t], sa[t], s3[q], sa[q])[0][0]
    assert asym >= 8


def test_sweep_pairs(O, mats):
    """the gapped sweep: every query length sits in the lane-group class the case table says, pair counts per query are odd"""
    s3, sa, pairs, kinds = MC.sweep_db()
    p = util.oracle_params(O, "-c 0.8 " + mats["directed"][2])
    lens = [len(x) for x in s3]
    per_q = {}
    for q, t in pairs:
        per_q[q] = per_q.get(q, 0) + 1
    assert all(v % 2 == 1 for v in per_q.values())
    assert sorted({lens[q] for q, _ in pairs}) == sorted(MC.SWEEP_QUERY_LENGTHS)
    for tab, g in MC.SWEEP_G.items():
        assert set(g.values()) == ({16, 32, 64} if tab < 3 else {64})
    for (q, t), kd in zip(pairs, kinds):
        if kd == "directed" and lens[q] <= 640:
            assert O.sw(s3[q], sa[q], s3[t], sa[t], p)[0] > 2 * O.sw(s3[t], sa[t], s3[q], sa[q], p)[0]


@pytest.mark.parametrize("name", ["hot", "mixed_hot", "negative"])
def test_hot_cases_leave_the_byte_field(O, mats, name):
    """the quantity the device keeps per DFS level in a biased field, counted in plain integers over the valid k-mers of the case database:
    64 + rest5 beyond 255 for every k-mer (hot), for a proper subset (mixed_hot); below 0 for k-mers that pass rest6 >= thr (negative)"""
    S3 = mats[name][0]
    s3 = MC.family_case_db()[0]
    opts = "-c 0.8 " + mats[name][2].split(" --mat-aa")[0]
    p = util.oracle_params(O, opts)
    r5, r6 = MC.rest5_plus_bias(s3, S3, p.pattern.decode())
    live = r6 >= p.kmer_thr
    over, under = int(((r5 > 255) & live).sum()), int(((r5 < 0) & live).sum())
    print(name, "k-mers", len(r5), "live", int(live.sum()), "over", over, "under", under, "thr", p.kmer_thr)
    if name == "hot":
        assert p.kmer_thr == 283 and over == len(r5) == 3597 and (r5 == 304).all()
    elif name == "mixed_hot":
        assert 100 <= over < int(live.sum()) - 100                                      # both kinds, plenty of each
    else:
        assert p.kmer_thr == -63 and under >= 100 and over == 0
    assert r5.min() >= 256 - 240 - 192 and (r5 - 64 + 256).min() >= 0 and (r5 - 64 + 256).max() < 1024      # ten bits biased by 256 hold every case
    ref = PC.oracle_prefilter(O, s3, opts, key="matrix_" + name)
    assert (ref["cnt"] > 0).sum() >= 20 and ref["totals"]["n_prefilter_hits"] >= 80
    if name == "hot":
        assert ref["totals"] == dict(n_sim_kmers=3597, n_kmer_hits=4427, n_candidates=88, n_prefilter_hits=88)


@pytest.mark.parametrize("pattern", LR.PATTERNS[1:], ids=LR.PATTERN_IDS[1:])
def test_closed_form_under_other_patterns(O, pattern):
    """hom_closed_form with span 6 and span 32 equals the oracle on a homopolymer sweep across the window edge"""
    span = len(pattern)
    lengths = MC.pattern_sweep_lengths(span)
    opts = "-c 0.8 --min-diag-hits 1 " + PC.ALL + " --spaced-kmer-pattern " + pattern
    p = util.oracle_params(O, opts)
    assert PC.pattern_offsets(p) == ([i for i, c in enumerate(pattern) if c == "1"], span)
    sdiag = int(p.S3[PC.HOM * 21 + PC.HOM])
    assert 6 * sdiag >= p.kmer_thr
    lists, n_hits, n_cand = PC.hom_closed_form(lengths, sdiag, span, p.min_diag_hits, p.min_ungapped, p.max_seqs)
    ref = PC.oracle_prefilter(O, PC.hom(lengths), opts, key=("pattern_sweep", pattern))
    assert ref["totals"]["n_kmer_hits"] == n_hits and ref["totals"]["n_candidates"] == n_cand
    assert [[(int(h["t"]), int(h["score"]), int(h["diag"])) for h in hl] for hl in ref["hits"]] == lists
    assert ref["cnt"][0] == 0 and ref["cnt"][1] == len(lengths) - 1                      # span - 1 residues: no k-mer; span residues: one


@pytest.mark.parametrize("pattern", LR.PATTERNS, ids=LR.PATTERN_IDS)
def test_x_variants_per_pattern(pattern):
    """which X variants leave valid k-mers depends on the offsets: counted here, relied on by the GPU test"""
    offs, span = [i for i, c in enumerate(pattern) if c == "1"], len(pattern)
    seq = np.full(3 * span + 7, PC.HOM, np.uint8)
    n = {v: len(PC.valid_kmer_positions(MC.with_x_for(seq, v, pattern), offs, span)) for v in MC.PATTERN_X_VARIANTS}
    full = len(seq) - span + 1
    assert n["plain"] == full and n["x_first"] == full - 1 and n["x_last"] == full - 1 and n["x_none_valid"] == 0
    assert (0 < n["x_every"] < full) if "0" in pattern else n["x_every"] == 0


def test_pattern_totals_on_the_family_database(O):
    """the three patterns give different hit lists on one database (the issue's figures)"""
    s3, _ = MC.family_case_db()
    got = [PC.oracle_prefilter(O, s3, "-c 0.8 --spaced-kmer-pattern " + pt, key=("family_pattern", pt))["totals"]["n_prefilter_hits"] for pt in LR.PATTERNS]
    assert got == [94, 93, 77], got
