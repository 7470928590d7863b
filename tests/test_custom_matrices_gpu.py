"""Every stage under substitution matrices with S(a, b) != S(b, a) (tests/matrix_cases.py: `directed`, `perturbed`, and the perturbation on one track
only), against the CPU oracle - exact integers.  Under a symmetric matrix a transposed index S[t * 21 + q] cannot be seen, and the three
optimisations that finalize_params' mat_symmetric switches off (shared DPs of mutual hits, the mirrored chunk walk of the prefilter, the symmetric
rank layout) are never off.  Here: the gapped kernels one pass at a time on one query length per lane-group width of every class table and the
long-query kernel, both backtrace routes, the whole pipeline stage by stage under six option sets, sharing switched off, the chunked prefilter with
one-way hits, virtual ranks, and clust.tsv / OUT.m8 bytes with the matrices passed on the command line.  MODE 6 (the shared start pass) is not
required here: its sharing semantics assume symmetric matrices.  The preconditions are proven on the CPU in tests/test_matrix_cases.py.

That these tests can fail was checked with five result-only, in-bounds mutations on a scratch copy (never committed), one library each, both new
modules run against it:
  the packed profile builder of uc_sw_pk_impl.hpp reading S3[c * 21 + q3] / SA[c * 21 + qa] -> 26 tests red: every sweep test under both matrices
      (forward / reverse / start, known-score re-run on tables 1 and 3, traceback statistics, backtraces), all ten stage-parity cases, both sharing
      cases, virtual ranks, and the three file tests;
  tb_walk_kernel's `sc` with the two letters exchanged -> test_traceback_statistics and test_backtraces_on_both_routes under both matrices,
      test_pipeline_stage_parity[* --min-seq-id 0.3] under both, test_search_m8_bytes_with_backtraces;
  ungapped_kernel with the two letters exchanged (all three loops) -> the eight k-mer-prefilter stage-parity cases (--prefilter-mode 1 has its own
      kernel and stays green), test_sharing_is_off...[only_s3], test_chunked_prefilter_keeps_one_way_hits;
  build_sim_tables reading S3[b * 21 + a] -> the same eight stage-parity cases, [only_s3], the chunked prefilter, virtual ranks and the three file tests;
  finalize_params testing only S3 for symmetry -> exactly test_sharing_is_off_when_either_track_is_asymmetric[only_sa] (mutual hits then share one
      DP and the second direction gets the first one's score: the records differ from the oracle's).
The whole module takes 6.7 s on an MI355X, oracle side included (27 tests, none above 0.7 s)."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bt_ref
import cluster_reassign_ref as RR
import dist_model as ucdist
import matrix_cases as MC
import ungapped_all_ref as XR
import util
from greedy_incremental_ref import greedy_incremental

pytestmark = pytest.mark.gpu

SW_PK_OVF = 0x7C00 - 256
EXE = os.path.join(util.ROOT, "bin", "unicore")


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.fixture(scope="module")
def mats(O, tmp_path_factory):
    d = tmp_path_factory.mktemp("matrices")
    return {name: MC.write_case(O, name, d)[2] for name in ("directed", "perturbed", "only_s3", "only_sa")}


def _pmap(fn, items):
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:
        return list(ex.map(fn, items))


def _engine(opts, s3, sa):
    import unicore_amd as U
    e = U.Engine(opts, verbosity=1)
    e.set_db(*util.flat(s3, sa))
    return e


# ---------------------------------------------------------------- 1: the gapped kernels, one pass at a time
@pytest.fixture(scope="module", params=["directed", "perturbed"])
def sweep(O, mats, request):
    s3, sa, pairs, kinds = MC.sweep_db()
    opts = "-c 0.8 " + mats[request.param]
    p = util.oracle_params(O, opts)
    odb = O.OracleDb(s3=s3, sa=sa)
    q = np.array([a for a, _ in pairs], np.uint32); t = np.array([b for _, b in pairs], np.uint32)
    n = len(q)
    fwd = np.array(_pmap(lambda i: O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p), range(n)), np.int64).reshape(n, 3)
    rev = np.array(_pmap(lambda i: O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p, rev_q=1)[0], range(n)), np.int64)
    pos = np.nonzero(fwd[:, 0] > 0)[0]

    def start(i):
        qe, te = fwd[i, 1], fwd[i, 2]
        return O.sw(s3[q[i]][: qe + 1], sa[q[i]][: qe + 1], s3[t[i]][: te + 1], sa[t[i]][: te + 1], p, rev_q=1, rev_t=1)
    st = np.array(_pmap(start, pos), np.int64).reshape(len(pos), 3)
    assert np.array_equal(st[:, 0], fwd[pos, 0])
    box = np.stack([fwd[pos, 1] - st[:, 1], fwd[pos, 1], fwd[pos, 2] - st[:, 2], fwd[pos, 2]], 1).astype(np.int32)
    tb = np.array(_pmap(lambda k: O.traceback(odb, p, q[pos[k]], t[pos[k]], *box[k]), range(len(pos))), np.int64).reshape(len(pos), 3)
    kinds = np.array(kinds)
    # the point of the case: the two orientations of a directed pair differ, so a transposed matrix index cannot give both right
    d, r = fwd[kinds == "directed", 0], fwd[kinds == "reverse", 0]
    assert (d != r).all() and len(pos) >= n - 4 and (fwd[:, 0] < SW_PK_OVF).all()
    lens = np.array([len(x) for x in s3])
    return dict(e=_engine(opts, s3, sa), p=p, s3=s3, sa=sa, q=q, t=t, n=n, fwd=fwd, rev=rev, pos=pos, st=st, box=box, tb=tb, kinds=kinds, lens=lens,
                name=request.param)


def test_forward_reverse_and_start_passes(sweep):
    """tables 0 (int32) and 1 (packed) in modes 0, 1, 2; queries beyond 2048 rows take the long-query kernel"""
    S = sweep
    e, q, t, pos = S["e"], S["q"], S["t"], S["pos"]
    ends = np.zeros((len(pos), 4), np.int32)
    ends[:, 1], ends[:, 3] = S["fwd"][pos, 1], S["fwd"][pos, 2]
    for tab in (0, 1):
        r = e.sw_pass(tab, 0, q, t)
        got = np.stack([r["score"], r["qe"], r["te"]], 1)
        assert np.array_equal(got, S["fwd"]), (tab, np.nonzero((got != S["fwd"]).any(1))[0][:10])
        cls_g = {}
        for L, c in zip(S["lens"][q], r["cls"]):
            cls_g.setdefault(int(L), set()).add(int(c))
        assert all(len(v) == 1 for v in cls_g.values())                 # one class per query length, the long queries in the class past the table
        assert np.array_equal(e.sw_pass(tab, 1, q, t)["score"], S["rev"]), tab
        r = e.sw_pass(tab, 2, q[pos], t[pos], box=ends)
        assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1), S["st"]), tab
    assert (S["lens"][q] == 2049).any()


@pytest.mark.parametrize("tab", [1, 3])
def test_known_score_end_rerun(sweep, tab):
    """MODE 4 (forward, optimum known) of the packed kernel, raw: the oracle's ends; table 3 (the sparse plans) forced"""
    S = sweep
    pos = S["pos"]
    r = S["e"].sw_pass(tab, 4, S["q"][pos], S["t"][pos], known=S["fwd"][pos, 0].astype(np.int32), raw=True)
    assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1), S["fwd"][pos]), tab


def test_traceback_statistics(sweep):
    """packed MODE 7 at bands 0 and 48 and the int32 MODE 3: (alignment length, identities, gap opens) of the oracle's traceback on its box"""
    S = sweep
    e, pos = S["e"], S["pos"]
    q, t, known = S["q"][pos], S["t"][pos], S["fwd"][pos, 0].astype(np.int32)
    for W in (0, 48):
        r = e.sw_pass(1, 7, q, t, box=S["box"], known=known, band=W)
        got = np.stack([r["aln_len"], r["idents"], r["gaps"]], 1)
        assert np.array_equal(got, S["tb"]), (W, np.nonzero((got != S["tb"]).any(1))[0][:10])
    r = e.sw_pass(2, 3, q, t, box=S["box"])
    assert np.array_equal(np.stack([r["aln_len"], r["idents"], r["gaps"]], 1), S["tb"])
    assert (S["tb"][:, 2] > 0).sum() >= 8


def test_backtraces_on_both_routes(sweep):
    """uc_engine_tb_emit_pass: the packed byte walk (banded and whole box) and the plain int32 DP, string for string against tests/bt_ref.py.  Under
    a directed matrix the I / D runs of (q, t) and (t, q) are not mirror images of each other"""
    S = sweep
    e, pos, s3, sa, p = S["e"], S["pos"], S["s3"], S["sa"], S["p"]
    S3, SA = bt_ref.matrices(p)
    q, t, known, box = S["q"][pos], S["t"][pos], S["fwd"][pos, 0].astype(np.int32), S["box"]

    def want_of(k):
        qs, qe, ts, te = box[k]
        return bt_ref.traceback(s3[q[k]][qs:qe + 1], sa[q[k]][qs:qe + 1], s3[t[k]][ts:te + 1], sa[t[k]][ts:te + 1], S3, SA, p.gap_open, p.gap_ext)
    want = [want_of(k) for k in range(len(pos))]
    assert all(w[4] == known[k] for k, w in enumerate(want))
    short = S["lens"][q] <= 2048

    def same(r, sel):
        for k, i in enumerate(sel):
            assert (r["aln_len"][k], r["idents"][k], r["gaps"][k], r["cigar"][k]) == want[i][:4], (i, int(q[i]), int(t[i]))
    sel = np.nonzero(short)[0]
    r = e.tb_emit_pass(1, q[sel], t[sel], box[sel], known[sel])
    assert not r["plain"].any() and not r["miss"].any()
    same(r, sel)
    r = e.tb_emit_pass(0, q[sel], t[sel], box[sel], known[sel], band=48)
    ok = r["miss"] == 0
    assert ok.sum() >= len(sel) - 4
    same({k: [v[j] for j in np.nonzero(ok)[0]] for k, v in r.items()}, sel[ok])
    r = e.tb_emit_pass(2, q[sel], t[sel], box[sel], known[sel])
    assert r["plain"].all()
    same(r, sel)
    sel = np.nonzero(~short)[0]
    assert len(sel) >= 3
    r = e.tb_emit_pass(3, q[sel], t[sel], box[sel], known[sel], band=48)
    assert r["plain"].all()
    same(r, sel)
    if S["name"] == "directed":
        cig = {(int(a), int(b)): w[3] for a, b, w in zip(q, t, want)}
        mirrored = [cig[a, b] == bt_ref.swap_id(cig[b, a]) for a, b in cig if (b, a) in cig and a < b]
        assert mirrored and not all(mirrored)


# ---------------------------------------------------------------- 2: the pipeline, stage by stage
def _case_db(name):
    if name == "directed":
        return MC.directed_db()
    return MC.family_case_db()


STAGE_OPTS = ["-c 0.8", "-c 0.5 --min-seq-id 0.3", "-c 0.8 --comp-bias-corr 1", "-c 0.8 --prefilter-mode 1", "-c 0.8 --cluster-mode 2 --cov-mode 1"]
ALN_FIELDS = ("score", "score_rev", "corrected", "pass_evalue", "accepted", "aln_len", "idents")


def _strip(opts, *flags):
    tok, out, i = opts.split(), [], 0
    while i < len(tok):
        if tok[i] in flags:
            i += 2
            continue
        out.append(tok[i]); i += 1
    return " ".join(out)


@pytest.mark.parametrize("opts", STAGE_OPTS)
@pytest.mark.parametrize("name", ["directed", "perturbed"])
def test_pipeline_stage_parity(O, mats, name, opts):
    """hit lists (target, score, diag in list order), the alignment records, the eight stage counters, the edges and both set covers equal the
    oracle's; the int32-only kernels give the same records"""
    import unicore_amd as U
    s3, sa = _case_db(name)
    full = opts + " " + mats[name]
    p = util.oracle_params(O, _strip(full, "--prefilter-mode", "--cluster-mode"))
    odb = O.OracleDb(s3=s3, sa=sa)
    e = _engine(full, s3, sa)
    e.prefilter()
    cnt, hits = e.hits()
    qh = np.repeat(np.arange(len(cnt)), cnt)
    if "--prefilter-mode 1" in opts:        # rule UC-1/X: the numpy restatement's lists, the oracle's record of every listed pair
        ids = list(range(len(s3)))
        sc, dg = XR.dense(O, s3, p, ids, ids)
        lists = XR.hit_lists(sc, dg, ids, p.min_ungapped, p.max_seqs, lens=[len(x) for x in s3], queries=ids)
        assert cnt.tolist() == [len(l) for l in lists]
        assert list(zip(hits["target"].tolist(), hits["score"].tolist(), hits["diag"].tolist())) == [h for l in lists for h in l]
        ms = [O.min_score(odb, p, a) for a in ids]
        ra = np.array([O.align_pair(odb, p, int(a), int(b), ms[int(a)]) for a, b in zip(qh, hits["target"])], O.ALN_DTYPE)
        counts = None
    else:
        ref = O.cluster(odb, p, threads=8)
        assert np.array_equal(cnt, ref["hit_cnt"])
        rh = np.concatenate([ref["hits"][i, : cnt[i]] for i in range(len(cnt))])
        for mine, theirs in (("target", "t"), ("score", "score"), ("diag", "diag")):
            assert np.array_equal(hits[mine], rh[theirs]), mine
        ra = np.concatenate([ref["aln"][i, : cnt[i]] for i in range(len(cnt))])
        counts = ref["counts"]
    e.align()
    al = e.alns()
    for f in ALN_FIELDS:
        assert np.array_equal(al[f], ra[f]), (f, np.nonzero(al[f] != ra[f])[0][:10])
    pe = al["pass_evalue"] == 1
    for f in ("qstart", "qend", "tstart", "tend"):
        assert np.array_equal(al[f][pe], ra[f][pe]), f
    acc = ra["accepted"] == 1
    pairs = set(zip(qh.tolist(), hits["target"].tolist()))
    if name == "directed" and counts is not None:      # one-way hits really occur in what was compared
        assert any((b, a) not in pairs for a, b in pairs)
    st = e.stats()
    if counts is not None:
        for a, b in (("n_sim_kmers", "n_sim_kmers"), ("n_kmer_hits", "n_kmer_hits"), ("n_candidates", "n_candidates"),
                     ("n_prefilter_hits", "n_prefilter_hits"), ("n_gapped_alignments", "n_alignments"), ("n_edges", "n_edges"),
                     ("cells_fwd", "cells_fwd"), ("cells_start", "cells_start")):
            assert st[a] == counts[b], (a, st[a], counts[b])
    else:
        assert st["n_prefilter_hits"] == len(hits) == st["n_gapped_alignments"]
    edges = e.edges()
    want_edges = {(int(a), int(b)) for a, b in zip(qh[acc], hits["target"][acc]) if a != b}
    assert {(int(a), int(b)) for a, b in edges.tolist() if a != b} == want_edges and want_edges
    if "--cluster-mode 2" in opts:
        lens = np.array([len(x) for x in s3], np.uint32)
        want = greedy_incremental(len(s3), edges, lens)
        assert np.array_equal(e.cluster_graph(edges, 2), want) and np.array_equal(U.cluster_graph(len(s3), edges, lens, 2), want)
    else:
        want = ref["assign"] if counts is not None else O.setcover(len(s3), edges)
        assert np.array_equal(U.setcover(e.n, edges), want) and np.array_equal(e.setcover(edges), want)
    assert len(set(np.asarray(want).tolist())) < e.n
    e2 = _engine(full + " --sw-kernel i32", s3, sa)
    e2.set_hits(cnt, hits)
    e2.align()
    assert e2.alns().tobytes() == al.tobytes()


@pytest.mark.parametrize("name", ["only_sa", "only_s3"])
def test_sharing_is_off_when_either_track_is_asymmetric(O, mats, name):
    """the same records with and without --sym-dedup 0, both the oracle's; and as many DP problems executed (n_sw_runs: mutual hits share one under
    sharing) - while under the shipped symmetric matrices the default executes fewer, so the figure does tell"""
    s3, sa = MC.family_case_db()
    p = util.oracle_params(O, "-c 0.8 " + mats[name])
    ref = O.cluster(O.OracleDb(s3=s3, sa=sa), p, threads=8)
    runs = {}
    for tag, opts in (("default", "-c 0.8 " + mats[name]), ("off", "-c 0.8 --sym-dedup 0 " + mats[name]), ("sym", "-c 0.8"), ("sym_off", "-c 0.8 --sym-dedup 0")):
        e = _engine(opts, s3, sa)
        e.reset_stats()
        e.prefilter(); e.align()
        st = e.stats()
        runs[tag] = (e.hits(), e.alns(), st["n_sw_runs"], st["cells_run"], st["cells_fwd"], st["cells_rev"])
    (cnt, hits), al = runs["default"][:2]
    assert np.array_equal(cnt, ref["hit_cnt"])
    ra = np.concatenate([ref["aln"][i, : cnt[i]] for i in range(len(cnt))])
    for f in ALN_FIELDS:
        assert np.array_equal(al[f], ra[f]), f
    assert runs["off"][1].tobytes() == al.tobytes() and runs["off"][0][1].tobytes() == hits.tobytes()
    assert runs["default"][2:] == runs["off"][2:], (runs["default"][2:], runs["off"][2:])
    assert runs["default"][4] == ref["counts"]["cells_fwd"] and runs["default"][5] == ref["counts"]["cells_rev"]
    assert runs["sym"][2] < runs["sym_off"][2] and runs["sym"][3] < runs["sym_off"][3]


def test_chunked_prefilter_keeps_one_way_hits(O, mats, tmp_path, monkeypatch):
    """>= 3 target chunks under the directed matrix: the lists equal the oracle's, one-way hits included - a mirrored pass over the upper
    triangle would invent the missing direction.  The full grid is walked: as many keys reach the sort as with the mirror switched off by hand"""
    s3, sa = MC.directed_db()
    opts = "-c 0.8 " + mats["directed"]
    ref = O.cluster(O.OracleDb(s3=s3, sa=sa), util.oracle_params(O, opts), threads=8, dumps=True)
    chunk = 400          # ten chunks; the base and the copy of the three longest families fall into different ones
    assert max(len(x) for x in s3) < chunk and sum(len(x) for x in s3) > 7 * chunk and len(s3[10]) + len(s3[11]) > chunk
    e = _engine(opts, s3, sa)
    out = {}
    for tag, env in (("one", {}), ("chunked", {"UC_PREFILTER_CHUNK_RES": str(chunk)}),
                     ("full", {"UC_PREFILTER_CHUNK_RES": str(chunk), "UC_PREFILTER_SYMMETRIC": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e.reset_stats()
        e.prefilter()
        out[tag] = (e.hits(), e.stats())
        for k in env:
            monkeypatch.delenv(k)
    for tag, ((cnt, hits), st) in out.items():
        assert np.array_equal(cnt, ref["hit_cnt"]), tag
        rh = np.concatenate([ref["hits"][i, : cnt[i]] for i in range(len(cnt))])
        assert np.array_equal(hits["target"], rh["t"]) and np.array_equal(hits["score"], rh["score"]) and np.array_equal(hits["diag"], rh["diag"]), tag
        for k in ("n_sim_kmers", "n_kmer_hits", "n_candidates", "n_prefilter_hits"):
            assert st[k] == ref["counts"][k], (tag, k)
    (cnt, hits), _ = out["chunked"]
    pairs = set(zip(np.repeat(np.arange(len(cnt)), cnt).tolist(), hits["target"].tolist()))
    assert any((b, a) not in pairs for a, b in pairs)
    assert out["chunked"][1]["n_filtered_hits"] == out["full"][1]["n_filtered_hits"]
    # the chunks are really taken at this size: under the SYMMETRISED matrix (max of both directions) the same cut walks the triangle, and fewer
    # keys reach the sort
    S3 = MC.matrices(O, "directed")[0]
    e2 = _engine("-c 0.8 --mat3di " + MC.write_matrix(str(tmp_path / "sym_3di.out"), np.maximum(S3, S3.T)), s3, sa)
    kept = {}
    for tag, env in (("triangle", {"UC_PREFILTER_CHUNK_RES": str(chunk)}), ("grid", {"UC_PREFILTER_CHUNK_RES": str(chunk), "UC_PREFILTER_SYMMETRIC": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e2.reset_stats()
        e2.prefilter()
        kept[tag] = e2.stats()["n_filtered_hits"]
        for k in env:
            monkeypatch.delenv(k)
    assert kept["triangle"] < kept["grid"]


def test_virtual_ranks_fall_back_to_the_full_grid(O, mats, tmp_path, monkeypatch):
    """three ranks, one target shard each: first the rank cells by hand (device-side export, union, merge == the unsharded lists; every pair owned by
    one rank; the union of the ranks' edges == the single engine's), then uc_cluster with three virtual ranks - the same clust.tsv as one rank and as
    the oracle, and exactly the work of the run with the symmetric layout switched off by hand"""
    import torch
    import unicore_amd as U
    s3, sa = MC.directed_db()
    opts = "-c 0.8 " + mats["directed"]
    lens = np.array([len(x) for x in s3])
    e = _engine(opts, s3, sa)
    e.prefilter()
    cnt_ref, hits_ref = e.hits()
    e.align()
    edges_ref = set(map(tuple, e.edges().tolist()))
    W, bufs = 3, []
    for tb, te, qb, qe in ucdist.grid_ranges(lens, W, W):
        e.prefilter(tb, te, qb, qe)
        n = e.hits_size()
        t = torch.empty((4, max(n, 1)), dtype=torch.int32, device="cuda")
        e.hits_export_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr())
        bufs.append(t[:, :n])
    allh = torch.cat(bufs, dim=1).contiguous()
    torch.cuda.synchronize()
    ptrs = [allh[i].data_ptr() for i in range(4)]
    ntot = int(allh.shape[1])
    assert e.hits_import_dev(ntot, *ptrs, 0, 1) == len(hits_ref)
    cnt, hits = e.hits()
    assert np.array_equal(cnt, cnt_ref) and hits.tobytes() == hits_ref.tobytes()
    total, edges = 0, set()
    for r in range(W):
        total += e.hits_import_dev(ntot, *ptrs, r, W)
        e.align()
        edges |= set(map(tuple, e.edges().tolist()))
    assert total == len(hits_ref) and edges == edges_ref and len(edges_ref) >= 8
    db = str(tmp_path / "db")
    util.write_db(db, s3, sa)
    monkeypatch.setenv("UC_VIRTUAL_GPUS", "1")
    res = {}
    for tag, n, env in (("g1", 1, {}), ("g3", 3, {}), ("g3_full", 3, {"UC_PREFILTER_SYMMETRIC": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        st = U.cluster(db, str(tmp_path / (tag + "_cluster")), str(tmp_path / "tmp"), opts + " --single-step-clustering", threads=4, num_gpus=n)
        for k in env:
            monkeypatch.delenv(k)
        U.createtsv(db, str(tmp_path / (tag + "_cluster")), str(tmp_path / (tag + ".tsv")))
        res[tag] = (open(str(tmp_path / (tag + ".tsv")), "rb").read(), st)
    odb = O.OracleDb(db)
    ref = O.cluster(odb, util.oracle_params(O, opts), threads=8, dumps=False)
    O.write_tsv(str(tmp_path / "ref.tsv"), odb, ref["assign"])
    want = open(str(tmp_path / "ref.tsv"), "rb").read()
    assert res["g1"][0] == want and res["g3"][0] == want and res["g3_full"][0] == want
    assert res["g3"][1]["n_gpus"] == 3 and res["g3"][1]["n_gapped_alignments"] == res["g1"][1]["n_gapped_alignments"] == ref["counts"]["n_alignments"]
    for k in ("n_kmer_hits", "n_filtered_hits", "n_sim_kmers"):
        assert res["g3"][1][k] == res["g3_full"][1][k], k


# ---------------------------------------------------------------- 3: files, the matrices on the command line
def test_default_workflow_tsv_bytes(O, mats, tmp_path):
    """`unicore cluster`-style default workflow (pre-step + cascade) with --mat3di / --mat-aa: clust.tsv == the oracle's cluster_workflow output"""
    import unicore_amd as U
    s3, sa = MC.directed_db()
    f3, fa = util.family_db(5, n_fam=5, members=4)
    s3, sa = s3 + f3, sa + fa
    db = str(tmp_path / "db")
    util.write_db(db, s3, sa)
    opts = "-c 0.8 " + mats["directed"]
    U.cluster(db, str(tmp_path / "clu"), str(tmp_path / "tmp"), opts, threads=4)
    U.createtsv(db, str(tmp_path / "clu"), str(tmp_path / "clu.tsv"))
    odb = O.OracleDb(db)
    p = util.oracle_params(O, opts)
    ref = O.cluster_workflow(odb, p, O.cascade_thresholds(p, 4.0, 3), linclust_m=20, threads=8)
    O.write_tsv(str(tmp_path / "ref.tsv"), odb, ref["assign"])
    got = open(str(tmp_path / "clu.tsv"), "rb").read()
    assert got == open(str(tmp_path / "ref.tsv"), "rb").read()
    util.tsv_invariants(str(tmp_path / "clu.tsv"), odb.names())
    assert len(set(ref["assign"].tolist())) < odb.n


def test_cluster_reassign_tsv_bytes(O, mats, tmp_path):
    """--cluster-reassign on the plain step under the directed matrix: the assignment of rule UC-1/R restated in tests/cluster_reassign_ref.py"""
    import unicore_amd as U
    s3, sa = MC.directed_db()
    db = str(tmp_path / "db")
    util.write_db(db, s3, sa)
    opts = "-c 0.8 --single-step-clustering --cluster-reassign " + mats["directed"]
    base, sw = RR.split_options(opts)
    p = util.oracle_params(O, base)
    odb = O.OracleDb(db)
    res = RR.reassign(O, U, odb, p, RR.workflow_assign(O, odb, p, sw), sw["cluster_mode"], sw["prefilter_mode"])
    assert not RR.unaccepted_members(O, odb, p, res)
    U.cluster(db, str(tmp_path / "clu"), str(tmp_path / "tmp"), opts, threads=4)
    U.createtsv(db, str(tmp_path / "clu"), str(tmp_path / "clu.tsv"))
    O.write_tsv(str(tmp_path / "ref.tsv"), odb, res["assign"])
    assert open(str(tmp_path / "clu.tsv"), "rb").read() == open(str(tmp_path / "ref.tsv"), "rb").read()
    print("reassign counts (verified, rejected, re-search pairs, clusters):", res["counts"])


def test_search_m8_bytes_with_backtraces(O, mats, tmp_path):
    """`unicore search -s "... -a"` with the directed matrix: OUT.m8 == the oracle's BLAST-tab file; the CIGAR column through convertalis equals
    tests/bt_ref.py's string of every row"""
    import unicore_amd as U
    s3, sa = MC.directed_db()
    qi, ti = list(range(0, 16, 2)), list(range(16))
    qdbp, tdbp = str(tmp_path / "q"), str(tmp_path / "t")
    util.write_db(qdbp, [s3[i] for i in qi], [sa[i] for i in qi], ["q_%02d" % i for i in qi])
    util.write_db(tdbp, s3, sa, ["t_%02d" % i for i in ti])
    opts = "-c 0.5 " + mats["directed"]
    out = str(tmp_path / "cli" / "hits")
    r = subprocess.run([EXE, "search", "--keep-aln-db", tdbp, qdbp, out, str(tmp_path / "tmp"), "-s", opts + " -a", "-v", "1"], capture_output=True,
                       text=True, env=dict(os.environ, UC_ALLOW_SYNTHETIC="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    qdb, tdb = O.OracleDb(qdbp), O.OracleDb(tdbp)
    po = util.oracle_params(O, "-e 10 --max-seqs 1000 " + opts)
    O.write_m8(str(tmp_path / "ref.m8"), qdb, tdb, po, O.search(qdb, tdb, po, threads=8))
    got = open(out + ".m8", "rb").read()
    assert got == open(str(tmp_path / "ref.m8"), "rb").read()
    rows = [l.split("\t") for l in got.decode().splitlines()]
    assert len(rows) >= 16 and {(r_[0], r_[1]) for r_ in rows} >= {("q_%02d" % i, "t_%02d" % (i + 1)) for i in qi}
    U.convertalis(qdbp, tdbp, out + "_aln", str(tmp_path / "bt.tsv"), format_output="query,target,cigar,qstart,qend,tstart,tend")
    S3, SA = bt_ref.matrices(po)
    k = 0
    for line in open(str(tmp_path / "bt.tsv")):
        qn, tn, cigar, qs, qe, ts, te = line.rstrip("\n").split("\t")
        a, b = int(qn[2:]), int(tn[2:])
        qs, qe, ts, te = int(qs) - 1, int(qe), int(ts) - 1, int(te)
        want = bt_ref.traceback(s3[a][qs:qe], sa[a][qs:qe], s3[b][ts:te], sa[b][ts:te], S3, SA, po.gap_open, po.gap_ext)
        assert cigar == want[3], (qn, tn)
        k += 1
    assert k == len(rows)
