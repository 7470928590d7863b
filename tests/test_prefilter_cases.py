"""The preconditions of tests/test_prefilter_kernels_gpu.py, proven on the CPU from the oracle and the closed form alone: every case really has the
shape that sends the device code down the path the GPU test is about (group sizes, ties, full lists, batch counts, run counts), and the two
references - the oracle and the closed form for homopolymers - agree with each other."""
import numpy as np
import pytest

import prefilter_cases as PC
import util


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _params(O, opts):
    p = util.oracle_params(O, opts)
    offs, span = PC.pattern_offsets(p)
    return p, offs, span, int(p.S3[PC.HOM * 21 + PC.HOM])


def _closed(O, lengths, opts):
    p, _, span, sdiag = _params(O, opts)
    return PC.hom_closed_form(lengths, sdiag, span, p.min_diag_hits, p.min_ungapped, p.max_seqs)


def _assert_oracle_is_closed_form(ref, closed):
    lists, n_hits, n_cand = closed
    assert ref["totals"]["n_kmer_hits"] == n_hits and ref["totals"]["n_candidates"] == n_cand
    assert ref["cnt"].tolist() == [len(l) for l in lists]
    for q, l in enumerate(lists):
        assert [(int(h["t"]), int(h["score"]), int(h["diag"])) for h in ref["hits"][q]] == l, q


def test_homopolymer_letter_qualifies(O):
    """the closed form needs the homopolymer's k-mer to be similar to itself: 6 * S3[c][c] >= kmer_thr at the default -s 4"""
    p, offs, span, sdiag = _params(O, "-c 0.8")
    assert p.kmer_thr == 29 and 6 * sdiag >= p.kmer_thr
    assert (offs, span) == ([0, 1, 3, 5, 8, 9], 10)
    assert sum(PC.HOM * 20 ** m for m in range(6)) in [int(v) for v in O.similar_kmers([PC.HOM] * 6, p.kmer_thr, p)]


@pytest.mark.parametrize("opts", PC.SWEEP_OPTS)
def test_window_sweep_preconditions(O, opts):
    """family 1: the oracle's hit total is the closed-form sum, and so are its lists; the groups reach every size class of the selection kernels"""
    ref = PC.oracle_prefilter(O, PC.hom(PC.SWEEP_LENGTHS), opts, key="sweep")
    n = [L - 9 for L in PC.SWEEP_LENGTHS]
    assert ref["totals"]["n_kmer_hits"] == sum(n) ** 2 == 5588496
    _assert_oracle_is_closed_form(ref, _closed(O, PC.SWEEP_LENGTHS, opts))
    sizes = sorted({a * b for a in n for b in n})
    assert sizes[0] == 1 and sizes[-1] == 6400 and max(n) == 80
    # the keys of one query are its groups one after the other: boundaries fall on every offset modulo 64 (the plain expansion keeps every key)
    ends = set()
    for a in n:
        e = 0
        for b in n:
            e += a * b
            ends.add(e % 64)
    assert ends == set(range(64))
    # shorter than a window / ending in the next window / covering the whole next window (deferred to diag_long_kernel) with runs across several windows
    assert any(s < 64 for s in sizes) and any(64 < s < 128 for s in sizes) and any(s >= 192 for s in sizes)
    # ties: against a longer target every diagonal in [Lq - Lt, 0] holds nq hits; the rule takes the smallest one, the mirrored pair the largest, 0
    assert sum(1 for d in range(-79, 1) if PC.hom_cnt(1, 80, d) == 1) == 80


def test_window_sweep_long_lengths_alone(O):
    """lengths 58 .. 89 alone: 4,260,096 hits, 1,024 candidates, every score saturated"""
    opts = PC.SWEEP_OPTS[1]
    ref = PC.oracle_prefilter(O, PC.hom(PC.SWEEP_LONG), opts, key="sweep_long")
    assert ref["totals"]["n_kmer_hits"] == 4260096 and ref["totals"]["n_candidates"] == 1024
    assert all((h["score"] == 255).all() for h in ref["hits"])
    _assert_oracle_is_closed_form(ref, _closed(O, PC.SWEEP_LONG, opts))


@pytest.mark.parametrize("lmax,n", PC.EXTREME_SETS)
def test_extreme_diagonal_preconditions(O, lmax, n):
    """family 2: the one-k-mer sequence against the longest one takes the most negative diagonal the biased field has to hold, the pair the other way
    round ties diagonal 0 with every diagonal up to lmax - 10.  The field widths are recomputed here by the rule of key_format() in uc_kmer_match.hip, not
    read from the engine (no statistic exposes them): what this shows is that the lengths and counts chosen sit on either side of a width change"""
    lengths = PC.extreme_lengths(lmax, n)
    assert len(lengths) == n and max(lengths) == lmax and lengths[0] == 10 and len(set(lengths)) == n
    dbits = 1
    while (1 << (dbits - 1)) < lmax:
        dbits += 1
    tbits = 1
    while (1 << tbits) < n:
        tbits += 1
    assert (dbits, tbits) == ({64: 7, 65: 8}[lmax], {32: 5, 33: 6}[n])
    opts = PC.SWEEP_OPTS[0]
    closed = _closed(O, lengths, opts)
    big = lengths.index(lmax)
    assert [r for r in closed[0][0] if r[0] == big][0][2] == -(lmax - 10)
    assert [r for r in closed[0][big] if r[0] == 0][0][2] == 0
    assert all(PC.hom_cnt(lmax - 9, 1, d) == 1 for d in range(0, lmax - 9))
    _assert_oracle_is_closed_form(PC.oracle_prefilter(O, PC.hom(lengths), opts, key=("extreme", lmax, n)), closed)


def test_tandem_repeat_preconditions(O):
    """family 3: a (query, target) group holds two diagonals whose counts differ by at most 1 and are both at least 64: several long competing runs"""
    s3 = PC.tandem_repeats()
    assert len(s3) == 46 and sum(len(s) for s in s3) < 10000
    ref = PC.oracle_prefilter(O, s3, PC.REPEAT_OPTS, key="repeat")
    _, offs, span, _ = _params(O, PC.REPEAT_OPTS)
    top = sorted(PC.exact_diagonal_counts(s3[22], s3[10], offs, span).values(), reverse=True)
    assert top[1] >= 64 and top[0] - top[1] <= 1, top[:4]
    assert ref["totals"]["n_candidates"] == 2 * 23 * 23 and ref["totals"]["n_kmer_hits"] > 3 << 20
    # the budgets of the driver variants: UC_HIT_CAP at its floor (2^20 keys) cuts >= 4 exact batches, UC_DRUN_MAX=8 is below the run lists of the distinct k-mers
    assert max(c["n_kmer_hits"] for c in ref["per_query"]) < 1 << 20
    assert PC.distinct_kmer_runs(O, s3, PC.REPEAT_OPTS) > 8


def test_sweep_driver_variant_preconditions(O):
    """family 6 on family 1: >= 4 exact batches at the floor of UC_HIT_CAP, >= 3 target chunks, none of them over the engine's density limit"""
    ref = PC.oracle_prefilter(O, PC.hom(PC.SWEEP_LENGTHS), PC.SWEEP_OPTS[0], key="sweep")
    assert ref["totals"]["n_kmer_hits"] > 3 << 20 and max(c["n_kmer_hits"] for c in ref["per_query"]) < 1 << 20
    for lengths, res in ((PC.SWEEP_LENGTHS, int(PC.SWEEP_CHUNK_RES)), ([len(s) for s in PC.tandem_repeats()], int(PC.REPEAT_CHUNK_RES))):
        chunks, cur = 1, 0
        for L in lengths:
            if cur and cur + L > res:
                chunks, cur = chunks + 1, 0
            cur += L
        assert chunks >= 3
    # (a homopolymer chunk of at most 400 residues has fewer than 400 target k-mer positions, so a query position has fewer than 400 hits in it and the
    # engine's density limit does not re-cut the chunks; that the chunking really survived is shown on the GPU: fewer expanded keys than the full grid)


def test_longest_sequence_preconditions(O):
    """family 4: the lists hold the diagonals +-65,495, which need dbits = 17 and the 16-bit position field to its last value"""
    s3 = PC.longest_pair()
    assert [len(s) for s in s3] == [65535, 65535, 40]
    ref = PC.oracle_prefilter(O, s3, PC.LONGEST_OPTS, key="longest")
    d = {(q, int(h["t"])): (int(h["diag"]), int(h["score"])) for q in range(3) for h in ref["hits"][q]}
    assert d[(0, 1)][0] == -65495 and d[(1, 0)][0] == 65495 and d[(1, 2)][0] == 65495 and d[(2, 1)][0] == -65495
    assert d[(0, 1)][1] == d[(1, 0)][1] >= 150 and ref["cnt"].tolist() == [3, 3, 3]


@pytest.mark.parametrize("max_seqs", [20, 1, 44])
def test_ties_at_the_cut_preconditions(O, max_seqs):
    """family 5: the lists of the 45 copies are full, every kept score is saturated: the survivors are decided by 'target ascending' alone"""
    s3, copies = PC.tied_copies()
    ref = PC.oracle_prefilter(O, s3, "-c 0.8 --max-seqs %d" % max_seqs, key="ties")
    assert sum(1 for q in copies if ref["cnt"][q] == max_seqs) == 45 >= 40 and copies[0] == 0
    assert ref["totals"]["n_candidates"] == 45 * 45 + 10 and ref["totals"]["n_prefilter_hits"] == 45 * max_seqs + 10
    for q in copies:
        assert ref["hits"][q]["t"].tolist() == copies[:max_seqs] and (ref["hits"][q]["score"] == 255).all() and (ref["hits"][q]["diag"] == 0).all()


def test_loaded_filter_preconditions(O):
    """family 7: the long query has at least 2^20 k-mer hits in more than 2,048 non-empty runs (several 2048-run tiles of filter_kernel)"""
    s3 = PC.loaded_filter(O)
    runs, hits = PC.query_runs(O, s3, len(s3) - 1, PC.LOADED_OPTS)
    assert hits >= 1 << 20 and runs > 2048, (runs, hits)
    ref = PC.oracle_prefilter(O, s3, PC.LOADED_OPTS, key="loaded")
    assert ref["per_query"][-1]["n_kmer_hits"] == hits == max(c["n_kmer_hits"] for c in ref["per_query"])
    print("loaded filter: %d hits, largest query %d hits in %d runs, oracle %.2f s" % (ref["totals"]["n_kmer_hits"], hits, runs, ref["seconds"]))


def test_saturating_filter_preconditions(O):
    """family 7, saturation: the long query's hits fall on at least 2^19 distinct (target, diagonal) keys - counted by numpy over similar_kmers against
    a sorted k-mer index, not by the oracle's E2 loop, whose hit total must agree.  Measured: 744,905 hits on 572,116 distinct keys; 38,023,899 hits in
    the whole case, oracle 2.7 s on 8 threads.  The whole database stays under the engine's density limit of 400 hits per query residue (333.5), so
    it is one index chunk and the query meets all its keys in ONE pass of filter_kernel."""
    s3 = PC.saturating_filter(O)
    hits, distinct = PC.query_keys(O, s3, len(s3) - 1, PC.SATURATING_OPTS)
    assert distinct >= 1 << 19, (hits, distinct)
    ref = PC.oracle_prefilter(O, s3, PC.SATURATING_OPTS, key="saturating")
    assert ref["per_query"][-1]["n_kmer_hits"] == hits < 1 << 32
    assert ref["totals"]["n_kmer_hits"] < 400 * sum(len(s) for s in s3)
    assert ref["params"].max_seqs > len(s3) and ref["params"].min_diag_hits == 2
    print("saturating filter: %d hits, long query %d hits on %d distinct keys, oracle %.2f s" % (ref["totals"]["n_kmer_hits"], hits, distinct, ref["seconds"]))


def test_x_variants_preconditions(O):
    """family 8: which X variants leave valid k-mers under the spaced pattern, and that a sequence without any is nobody's target and has no list"""
    _, offs, span, _ = _params(O, "-c 0.8")
    for name, (s3, variant, opts) in PC.x_cases().items():
        ref = PC.oracle_prefilter(O, s3, opts, key=name)
        nv = [len(PC.valid_kmer_positions(s, offs, span)) for s in s3]
        targets = set(int(t) for h in ref["hits"] for t in h["t"])
        for i, v in enumerate(variant):
            L = len(s3[i])
            assert nv[i] == {"plain": L - 9, "x_first": L - 10, "x_last": L - 10, "x_none_valid": 0}.get(v, nv[i]), (name, i, v)
            if v == "x_every10":
                assert 0 < nv[i] < L - 9        # the X falls on a skipped pattern position in four of every ten windows
            if v == "x_none_valid":
                assert i not in targets and ref["cnt"][i] == 0
            else:
                assert i in targets and ref["cnt"][i] > 0
        if name == "x_hom":      # below the saturation at 255: an X inside the overlap shows in the score
            assert max(int(h["score"].max()) for h in ref["hits"] if len(h)) < 255
            plain = [i for i, v in enumerate(variant) if v == "plain"]
            xf = [i for i, v in enumerate(variant) if v == "x_first"]
            self_score = lambda i: int(ref["hits"][i]["score"][ref["hits"][i]["t"] == i][0])
            assert all(self_score(b) < self_score(a) for a, b in zip(plain, xf))
        # the X variants are scored as E3 partners: an X inside the overlap changes the score of the pair, not its membership
        assert ref["totals"]["n_candidates"] == ref["totals"]["n_prefilter_hits"] > 0
