"""Rule UC-1/X (--prefilter-mode 1) on the GPU: the all-diagonals kernel, the hit lists, cluster and search end to end, all against the numpy
restatement of tests/ungapped_all_ref.py (itself checked against the oracle in test_prefilter_mode1.py) and the oracle's gapped pieces."""
import os

import numpy as np
import pytest

import bt_ref
import ungapped_all_ref as R
import util

pytestmark = pytest.mark.gpu
NQ = 64                        # the kernel test's queries: sequences [0, NQ) against all 128
PAIR_BYTES = 53                # what the tile budget counts per pair (UNGAPPED_ALL_PAIR_BYTES: tile 5 + candidate record 16 + selection arrays 32)
GOLD_C1 = os.path.join(util.ROOT, "tests", "golden", "c1", "db")


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    oracle_py.lib()
    return oracle_py


@pytest.fixture(scope="module")
def db():
    s3, sa, info = R.mode1_db()
    return dict(s3=s3, sa=sa, info=info, n=len(s3))


@pytest.fixture(scope="module")
def expected(O, db):
    """dense restatement per option string, computed once per session"""
    cache = {}

    def get(opts, nq):
        key = (opts, nq)
        if key not in cache:
            cache[key] = R.dense(O, db["s3"], util.oracle_params(O, opts), list(range(nq)), list(range(db["n"])))
        return cache[key]
    return get


def _engine(opts, db):
    import unicore_amd as U
    e = U.Engine(opts, verbosity=1, device=0)
    e.set_db(*util.flat(db["s3"], db["sa"]))
    return e


def _lists(e, qend=None):
    cnt, hits = e.hits()
    out, k = [], 0
    for q in range(e.n if qend is None else qend):
        out.append([(int(h["target"]), int(h["score"]), int(h["diag"])) for h in hits[k:k + int(cnt[q])]])
        k += int(cnt[q])
    return out


@pytest.mark.parametrize("bias", ["", " --comp-bias-corr 1"])
def test_kernel_scores_and_diagonals(db, expected, bias):
    """every (query, target) pair of 64 x 128: length 1, below the span, 50-400, ~5,000, X residues, an identical pair, the capped periodic pair"""
    want_s, want_d = expected(bias.strip(), NQ)
    e = _engine("-c 0.8 --prefilter-mode 1" + bias, db)
    got_s, got_d = e.ungapped_all(0, NQ, 0, db["n"])
    bad = np.argwhere((got_s != want_s) | (got_d != want_d))
    print("pairs %d, mismatches %d, capped pairs %d" % (want_s.size, len(bad), int((want_s == 255).sum())))
    assert len(bad) == 0, [(int(q), int(t), int(got_s[q, t]), int(want_s[q, t]), int(got_d[q, t]), int(want_d[q, t])) for q, t in bad[:8]]
    a, b = db["info"]["periodic"]
    assert want_s[a, b] == 255 and want_s[3, 4] == want_s[3, 3]
    # the empty sequence: score 0, diag 0 as a query and as a target
    z = db["info"]["empty"]
    assert len(db["s3"][z]) == 0 and not got_s[z].any() and not got_d[z].any() and not got_s[:, z].any() and not got_d[:, z].any()
    # a tiny tile budget: several query batches and target chunks (23 x 23 pairs per tile), a sub-range, and one query per batch (the empty one alone)
    s2, d2 = e.ungapped_all(0, NQ, 0, db["n"], tile_bytes=PAIR_BYTES * 23 * 23)
    assert np.array_equal(s2, want_s) and np.array_equal(d2, want_d)
    s3_, d3 = e.ungapped_all(5, 31, 17, 99, tile_bytes=PAIR_BYTES * 7 * 7)
    assert np.array_equal(s3_, want_s[5:31, 17:99]) and np.array_equal(d3, want_d[5:31, 17:99])
    s4, d4 = e.ungapped_all(5, 31, 0, 20, tile_bytes=PAIR_BYTES)
    assert np.array_equal(s4, want_s[5:31, 0:20]) and np.array_equal(d4, want_d[5:31, 0:20])


@pytest.mark.parametrize("opts", ["", " --max-seqs 20", " --comp-bias-corr 1 --max-seqs 50"])
def test_hit_lists(O, db, expected, opts, monkeypatch):
    """Engine.prefilter under mode 1 == threshold + sort + truncate of the restatement, max_seqs above and below the number of passing targets,
    whatever the tile budget; the counters follow the rule"""
    full = "-c 0.8 --prefilter-mode 1" + opts
    ref_opts = " ".join(t for t in opts.replace("--max-seqs 20", "").replace("--max-seqs 50", "").split())
    p = util.oracle_params(O, ref_opts)
    max_seqs = 20 if "20" in opts else 50 if "50" in opts else p.max_seqs
    want_s, want_d = expected(ref_opts, db["n"])
    want = R.hit_lists(want_s, want_d, list(range(db["n"])), p.min_ungapped, max_seqs)
    passing = [(want_s[q] >= p.min_ungapped).sum() for q in range(db["n"])]
    assert (max(passing) > max_seqs) == bool(opts) and max(passing) > 20
    e = _engine(full, db)
    e.prefilter()
    got = _lists(e)
    assert got == want
    st = e.stats()
    assert st["n_sim_kmers"] == 0 and st["n_kmer_hits"] == 0
    assert st["n_candidates"] == db["n"] * db["n"] and st["n_prefilter_hits"] == sum(len(w) for w in want)
    monkeypatch.setenv("UC_UNGAPPED_TILE_BYTES", str(PAIR_BYTES * 19 * 19))          # 7 query batches x 7 target chunks
    e2 = _engine(full, db)
    e2.prefilter()
    assert _lists(e2) == want
    monkeypatch.delenv("UC_UNGAPPED_TILE_BYTES")
    e3 = _engine(full, db)                                                   # a query range against a target range
    e3.prefilter(10, 100, 3, 40)
    sub = R.hit_lists(want_s[3:40, 10:100], want_d[3:40, 10:100], list(range(10, 100)), p.min_ungapped, max_seqs)
    assert _lists(e3)[3:40] == sub


def test_empty_sequence_is_in_no_hit_list(O, db, expected):
    """a zero-length database entry never scores and is never listed, even when the threshold lets score 0 through (and one pair per tile)"""
    want_s, want_d = expected("", db["n"])
    lens = [len(s) for s in db["s3"]]
    z = db["info"]["empty"]
    want = R.hit_lists(want_s, want_d, list(range(db["n"])), 0, 300, lens=lens)
    assert want[z] == [] and all(t != z for l in want for t, _, _ in l) and all(len(want[q]) == db["n"] - 1 for q in range(db["n"]) if q != z)
    e = _engine("-c 0.8 --prefilter-mode 1 --min-ungapped-score 0", db)
    e.prefilter()
    assert _lists(e) == want
    e.prefilter(z, z + 1, 6, z + 1)                         # the empty target alone: nothing
    assert e.hits_size() == 0


def test_short_query_is_found_only_by_mode_1(db):
    """a 6-residue sequence (shorter than the k-mer span) that is a substring of two others: no k-mer, no hit under mode 0; found under mode 1"""
    s, inside = db["info"]["short"], db["info"]["identical"]
    assert len(db["s3"][s]) == 6
    e0 = _engine("-c 0.8", db)
    e0.prefilter()
    l0 = _lists(e0)
    assert l0[s] == [] and all(t != s for q in range(db["n"]) for t, _, _ in l0[q])
    e1 = _engine("-c 0.8 --prefilter-mode 1", db)
    e1.prefilter()
    l1 = _lists(e1)
    found = {t: (sc, d) for t, sc, d in l1[s]}
    assert inside[0] in found and inside[1] in found and s in found
    assert found[inside[0]][1] == -40 and found[inside[0]][0] == found[s][0]        # the substring starts at target position 40; as good as the self hit


def test_mode_0_is_untouched(db):
    """an explicit --prefilter-mode 0 is today's prefilter: same lists, same counters"""
    res = []
    for opts in ("-c 0.8", "-c 0.8 --prefilter-mode 0"):
        e = _engine(opts, db)
        e.prefilter()
        st = e.stats()
        res.append((_lists(e), {k: st[k] for k in ("n_sim_kmers", "n_kmer_hits", "n_candidates", "n_prefilter_hits")}))
    assert res[0] == res[1] and res[0][1]["n_kmer_hits"] > 0


def test_mode_1_contains_mode_0_at_size():
    """tests/golden/c1 with max_seqs >= n: every (q, t) of the k-mer lists is in the exhaustive lists with a score no lower (the k-mer candidate's diagonal is
    one of the diagonals scanned)"""
    import unicore_amd as U
    lists = []
    for mode in (0, 1):
        e = U.Engine("-c 0.8 --max-seqs 1000 --prefilter-mode %d" % mode, verbosity=1, device=0)
        e.load_db(GOLD_C1)
        assert e.n <= 1000
        e.prefilter()
        lists.append(_lists(e))
    n0 = 0
    for q, (l0, l1) in enumerate(zip(*lists)):
        s1 = {t: sc for t, sc, _ in l1}
        for t, sc, _ in l0:
            assert t in s1 and s1[t] >= sc, (q, t)
            n0 += 1
    assert n0 > 0 and sum(len(l) for l in lists[1]) > n0                          # the check is not vacuous, and mode 1 finds more


E2E = "-c 0.8 --min-ungapped-score 25 --prefilter-mode 1"
E2E_REF = "-c 0.8 --min-ungapped-score 25"


@pytest.fixture(scope="module")
def on_disk(db, tmp_path_factory):
    d = tmp_path_factory.mktemp("pm1")
    names = util.write_db(str(d / "db"), db["s3"], db["sa"])
    return dict(dir=str(d), prefix=str(d / "db"), names=names)


@pytest.fixture(scope="module")
def gapped(O, db, expected):
    """the oracle's E5/E6 record of every pair of the expected hit lists under E2E_REF: {(q, t): record}"""
    p = util.oracle_params(O, E2E_REF)
    odb = O.OracleDb(s3=db["s3"], sa=db["sa"])
    want_s, want_d = expected("", db["n"])
    lists = R.hit_lists(want_s, want_d, list(range(db["n"])), p.min_ungapped, p.max_seqs)
    rec = {}
    for q, l in enumerate(lists):
        ms = O.min_score(odb, p, q)
        for t, _, _ in l:
            rec[(q, t)] = O.align_pair(odb, p, q, t, ms)
    return dict(p=p, odb=odb, rec=rec)


@pytest.fixture(scope="module")
def single_step(on_disk):
    """uc_cluster --single-step-clustering under mode 1 on one rank: (path of its clust.tsv, stats)"""
    import unicore_amd as U
    d = on_disk["dir"]
    st = U.cluster(on_disk["prefix"], d + "/s1_cluster", d + "/tmp", E2E + " --single-step-clustering")
    U.createtsv(on_disk["prefix"], d + "/s1_cluster", d + "/s1.tsv")
    return d + "/s1.tsv", st


def test_cluster_single_step_equals_the_oracle_pieces(O, db, on_disk, gapped, single_step):
    """uc_cluster --single-step-clustering --prefilter-mode 1: clust.tsv == align_pair over the expected lists -> setcover -> write_tsv, byte for byte"""
    import unicore_amd as U
    d = on_disk["dir"]
    edges = [(q, t) for (q, t), a in sorted(gapped["rec"].items()) if a["accepted"]]
    assert len(edges) > db["n"]
    assign = O.setcover(db["n"], np.array(edges, np.uint32))
    odb = O.OracleDb(prefix=on_disk["prefix"])
    O.write_tsv(d + "/want.tsv", odb, assign)
    s1, st = single_step
    assert open(s1, "rb").read() == open(d + "/want.tsv", "rb").read()
    assert st["n_kmer_hits"] == 0 and st["n_candidates"] == db["n"] ** 2
    # the 6-residue sequence is no singleton by construction of the prefilter any more - and whatever the gapped stage decides, the file is valid
    util.tsv_invariants(s1, on_disk["names"])


def test_cluster_default_workflow_one_and_two_ranks(on_disk, single_step, monkeypatch):
    """pre-step + cascade under mode 1: runs, gives a valid clust.tsv, and the same bytes on 1 rank and on 2 (virtual) ranks"""
    import unicore_amd as U
    d = on_disk["dir"]
    U.cluster(on_disk["prefix"], d + "/w1_cluster", d + "/tmp", E2E, threads=4, num_gpus=1)
    U.createtsv(on_disk["prefix"], d + "/w1_cluster", d + "/w1.tsv")
    util.tsv_invariants(d + "/w1.tsv", on_disk["names"])
    monkeypatch.setenv("UC_VIRTUAL_GPUS", "1")
    for tag, opts, n in (("w2", E2E, 2), ("s2", E2E + " --single-step-clustering", 2)):
        st = U.cluster(on_disk["prefix"], d + "/%s_cluster" % tag, d + "/tmp", opts, threads=4, num_gpus=n)
        assert st["n_gpus"] == n
        U.createtsv(on_disk["prefix"], d + "/%s_cluster" % tag, d + "/%s.tsv" % tag)
    assert open(d + "/w2.tsv", "rb").read() == open(d + "/w1.tsv", "rb").read()
    assert open(d + "/s2.tsv", "rb").read() == open(single_step[0], "rb").read()


def _read_aln_db(prefix):
    data = open(prefix, "rb").read()
    rows = {}
    for line in open(prefix + ".index"):
        k, off, ln = (int(x) for x in line.split())
        rows[k] = [r.split("\t") for r in data[off:off + ln].rstrip(b"\0").decode().splitlines()]
    return rows


def test_search_and_convertalis(O, db, on_disk, gapped):
    """uc_search (+ -a) under mode 1, database against itself: per query the targets, coordinates, alignment length and CIGAR of the records built from
    align_pair / the traceback restatement over the expected hits"""
    import unicore_amd as U
    d, pre = on_disk["dir"], on_disk["prefix"]
    p = gapped["p"]
    S3, SA = bt_ref.matrices(p)
    so = E2E + " -e %g" % p.evalue                  # (`search` has its own default E-value: the records of `gapped` are those of the cluster default)
    U.search(pre, pre, d + "/plain_aln", d + "/tmp", so)
    U.search(pre, pre, d + "/bt_aln", d + "/tmp", so + " -a")
    plain, rows = _read_aln_db(d + "/plain_aln"), _read_aln_db(d + "/bt_aln")
    assert {k: [f[:14] for f in rr] for k, rr in rows.items()} == plain
    n = 0
    for q in range(db["n"]):
        want = {t: a for (qq, t), a in gapped["rec"].items() if qq == q and a["accepted"]}
        got = {int(f[0]): f for f in rows.get(q, [])}
        assert sorted(got) == sorted(want), q
        for t, f in got.items():
            a = want[t]
            box = (int(a["qstart"]), int(a["qend"]), int(a["tstart"]), int(a["tend"]))
            assert (int(f[4]), int(f[5]), int(f[7]), int(f[8])) == box, (q, t)
            ln, idn, gp = O.traceback(gapped["odb"], p, q, t, *box)
            assert int(f[10]) == ln, (q, t)
            qs, qe, ts, te = box
            if (qe - qs + 1) * (te - ts + 1) <= 400 * 400:                       # the python traceback restatement: all but the long self hit
                tb = bt_ref.traceback(db["s3"][q][qs:qe + 1], db["sa"][q][qs:qe + 1], db["s3"][t][ts:te + 1], db["sa"][t][ts:te + 1], S3, SA, p.gap_open, p.gap_ext)
                assert (int(f[10]), f[14]) == (tb[0], tb[3]), (q, t)
            n += 1
    assert n > db["n"]
    U.convertalis(pre, pre, d + "/bt_aln", d + "/bt.tsv", format_output="query,target,qstart,qend,tstart,tend,alnlen,cigar")
    k = 0
    for line in open(d + "/bt.tsv"):
        qn, tn, qs, qe, ts, te, alen, cigar = line.rstrip("\n").split("\t")
        q, t = on_disk["names"].index(qn), on_disk["names"].index(tn)
        f = {int(r[0]): r for r in rows[q]}[t]
        assert (int(qs) - 1, int(qe) - 1, int(ts) - 1, int(te) - 1, alen, cigar) == (int(f[4]), int(f[5]), int(f[7]), int(f[8]), f[10], f[14])
        k += 1
    assert k == n


def test_clis_take_the_flag(on_disk, single_step):
    """bin/unicore cluster -c / search -s and bin/foldseek cluster / search forward the option string"""
    import subprocess
    d, pre = on_disk["dir"], on_disk["prefix"]
    uni, shim = os.path.join(util.ROOT, "bin", "unicore"), os.path.join(util.ROOT, "bin", "foldseek")
    env = dict(os.environ, UC_ALLOW_SYNTHETIC="1")
    run = lambda argv: subprocess.run(argv, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600, check=True)
    run([uni, "cluster", "-c", E2E + " --single-step-clustering", pre, d + "/cli_clu", d + "/tmp"])
    run([shim, "cluster", pre, d + "/shim_cluster", d + "/tmp", "--single-step-clustering"] + E2E.split())
    run([shim, "createtsv", pre, pre, d + "/shim_cluster", d + "/shim.tsv"])
    assert open(d + "/cli_clu.tsv", "rb").read() == open(d + "/shim.tsv", "rb").read() != b""
    assert open(d + "/shim.tsv", "rb").read() == open(single_step[0], "rb").read()
    run([uni, "search", "-s", E2E, pre, pre, d + "/cli_search", d + "/tmp"])
    run([shim, "search", pre, pre, d + "/shim_aln", d + "/tmp"] + E2E.split())
    run([shim, "convertalis", pre, pre, d + "/shim_aln", d + "/shim.m8"])
    assert open(d + "/cli_search.m8").read() == open(d + "/shim.m8").read() != ""
    r = subprocess.run([shim, "cluster", pre, d + "/bad_cluster", d + "/tmp", "--prefilter-mode", "2"], env=env, capture_output=True, timeout=600)
    assert r.returncode != 0
