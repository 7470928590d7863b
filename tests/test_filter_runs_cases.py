"""The preconditions of tests/test_filter_runs_gpu.py, proven on the CPU by brute force over the 64 k-mers of a two-letter alphabet, the oracle and
the closed form for homopolymers: every case really has the shape at which the indexing of a query's runs through the plan can go wrong - a run list
across a tile boundary, one list shared by all positions, zero-run positions inside a query's range, queries without runs, batches and super-batches
that start behind the first position of the plan."""
import numpy as np
import pytest

import filter_runs_cases as FC
import prefilter_cases as PC
import util


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _kmers_present(O, s3, opts):
    p = util.oracle_params(O, opts)
    offs, span = PC.pattern_offsets(p)
    return {tuple(int(s[i + o]) for o in offs) for s in s3 for i in PC.valid_kmer_positions(s, offs, span)}


def test_case_a_a_run_list_straddles_the_tile_boundary(O):
    """A: the long query has > 2,048 runs, every position holds several, and the list of one position begins before run 2,048 and ends behind it; the
    query fits the LDS prefix whole (<= FILTER_PW positions: no sampled search)"""
    s3 = FC.case_a(O)
    assert [len(s) for s in s3] == FC.A_LENGTHS and len(s3[FC.A_LONG]) == 300 <= FC.FILTER_PW
    assert _kmers_present(O, s3, FC.OPTS) == FC.all_two_letter_kmers(O)
    runs, hits = FC.position_runs(O, s3, FC.OPTS)
    r = runs[FC.A_LONG]
    assert r.sum() > FC.TILE_RUNS and (r[:291] >= 2).all() and (r[291:] == 0).all()
    pre = np.concatenate([[0], np.cumsum(r)])
    straddling = [i for i in range(len(r)) if pre[i] < FC.TILE_RUNS < pre[i + 1]]
    assert len(straddling) == 1, pre[90:96]
    assert sum(int(x.sum()) for x in runs) > 4 * FC.TILE_RUNS
    # the brute-force counts are the oracle's: hits per query
    ref = PC.oracle_prefilter(O, s3, FC.OPTS, key="fr_a")
    assert [c["n_kmer_hits"] for c in ref["per_query"]] == [int(h.sum()) for h in hits]
    print("case A: long query %d runs, run 2048 inside the list of position %d (runs %d .. %d); %d hits in all" % (
        r.sum(), straddling[0], pre[straddling[0]], pre[straddling[0] + 1] - 1, ref["totals"]["n_kmer_hits"]))


def test_case_a_two_target_chunks_under_the_density_limit(O):
    """E: UC_PREFILTER_CHUNK_RES cuts case A into two target chunks, and neither is so dense (400 k-mer hits per query residue) that the driver would
    re-cut the range into one chunk again: the hits of ALL queries in one chunk's targets, over all query residues"""
    s3 = FC.case_a(O)
    chunks = FC.target_chunks(FC.A_LENGTHS, int(FC.A_CHUNK_RES))
    assert len(chunks) == 2 and chunks[0][0] == 0 and chunks[1][1] == len(s3)
    assert chunks[0][0] <= FC.A_LONG < chunks[0][1]            # the long query lies in the first chunk: the second pass meets it as a mirrored query only
    p = util.oracle_params(O, FC.OPTS)
    offs, span = PC.pattern_offsets(p)
    for b, e in chunks:
        occ = {}
        for s in s3[b:e]:
            for i in PC.valid_kmer_positions(s, offs, span):
                k = tuple(int(s[i + o]) for o in offs)
                occ[k] = occ.get(k, 0) + 1
        val = {sum(c * 20 ** m for m, c in enumerate(k)): n for k, n in occ.items()}
        hits = 0
        for s in s3:
            for i in PC.valid_kmer_positions(s, offs, span):
                k = [int(s[i + o]) for o in offs]
                hits += sum(val.get(int(v), 0) for v in O.similar_kmers(k, p.kmer_thr, p))
        assert hits < 400 * sum(FC.A_LENGTHS), (b, e, hits)


def test_case_b_one_list_for_every_position(O):
    """B: one distinct k-mer with one run; the long homopolymer has > 2,048 k-mer positions, i.e. > 2,048 runs that are all the same list, and more
    positions than the LDS prefix holds (the sampled search); the oracle agrees with the closed form"""
    s3 = FC.case_b()
    assert len(_kmers_present(O, s3, FC.OPTS)) == 1
    runs, _ = FC.position_runs(O, s3, FC.OPTS)
    assert all(set(r[:len(r) - 9].tolist()) == {1} for r in runs)
    assert runs[FC.B_LONG].sum() == 2091 > FC.TILE_RUNS and len(s3[FC.B_LONG]) > 2 * FC.FILTER_PW
    p = util.oracle_params(O, FC.OPTS)
    sdiag = int(p.S3[PC.HOM * 21 + PC.HOM])
    lists, n_hits, n_cand = PC.hom_closed_form(FC.B_LENGTHS, sdiag, 10, p.min_diag_hits, p.min_ungapped, p.max_seqs)
    ref = PC.oracle_prefilter(O, s3, FC.OPTS, key="fr_b")
    assert ref["totals"]["n_kmer_hits"] == n_hits == sum(L - 9 for L in FC.B_LENGTHS) ** 2 and ref["totals"]["n_candidates"] == n_cand
    for q, l in enumerate(lists):
        assert [(int(h["t"]), int(h["score"]), int(h["diag"])) for h in ref["hits"][q]] == l, q
    # under UC_HIT_CAP at its floor the long query is a batch of its own that starts behind the first position of the plan
    per_q = [c["n_kmer_hits"] for c in ref["per_query"]]
    assert per_q[FC.B_LONG] > FC.HIT_CAP_FLOOR and FC.B_LONG > 0 and sum(per_q[:FC.B_LONG]) < FC.HIT_CAP_FLOOR


def test_case_c_positions_and_queries_without_runs(O):
    """C: the gapped queries have zero-run positions at the start, a stretch of them longer than a k-mer's span in the middle and at the end, with
    run-holding positions on either side of each; they still span several tiles; the dead query has no run at all and lies between two that have"""
    s3 = FC.case_c(O)
    runs, _ = FC.position_runs(O, s3, FC.OPTS)
    p = util.oracle_params(O, FC.OPTS)
    _, span = PC.pattern_offsets(p)
    for q in FC.C_GAPPED:
        r = runs[q]
        nz = np.nonzero(r)[0]
        assert r[0] == 0 and nz[0] >= 3 and nz[-1] < len(r) - span - 1
        inner = r[nz[0]:nz[-1] + 1]
        zero_stretch = max(len(z) for z in "".join("0" if x == 0 else "1" for x in inner).split("1"))
        assert zero_stretch > span, zero_stretch
    assert runs[FC.C_GAPPED[0]].sum() > FC.TILE_RUNS
    assert runs[FC.C_DEAD].sum() == 0 and runs[FC.C_DEAD - 1].sum() > 0 and runs[FC.C_DEAD + 1].sum() > 0
    ref = PC.oracle_prefilter(O, s3, FC.OPTS, key="fr_c")
    assert ref["cnt"][FC.C_DEAD] == 0 and all(ref["cnt"][q] > 0 for q in range(len(s3)) if q != FC.C_DEAD)
    assert FC.C_DEAD not in set(int(t) for h in ref["hits"] for t in h["t"])


def test_case_d_batch_and_super_batch_cuts(O):
    """D: the preconditions of the batch cuts (as test_batch_cuts_change_nothing's): more than 3 x 2^20 k-mer hits and every query below 2^20, so
    UC_HIT_CAP=1048576 gives >= 4 exact batches; the distinct k-mers have far more than 8 runs, so UC_DRUN_MAX=8 cuts the super-batch.  Case D is case A
    with 15 more sequences: the long query still has a list across run 2,048"""
    a, s3 = FC.case_a(O), FC.case_d(O)
    assert all(np.array_equal(x, y) for x, y in zip(a, s3)) and len(s3) == len(a) + 15
    ref = PC.oracle_prefilter(O, s3, FC.OPTS, key="fr_d")
    per_q = [c["n_kmer_hits"] for c in ref["per_query"]]
    assert ref["totals"]["n_kmer_hits"] > 3 * FC.HIT_CAP_FLOOR and max(per_q) < FC.HIT_CAP_FLOOR, (ref["totals"]["n_kmer_hits"], max(per_q))
    assert sum(per_q[:FC.A_LONG]) > 0                           # queries before the long one: it never starts a plan
    assert PC.distinct_kmer_runs(O, s3, FC.OPTS) > 8
    runs, _ = FC.position_runs(O, s3, FC.OPTS)
    pre = np.concatenate([[0], np.cumsum(runs[FC.A_LONG])])
    assert any(pre[i] < FC.TILE_RUNS < pre[i + 1] for i in range(len(pre) - 1))
    print("case D: %d hits, largest query %d" % (ref["totals"]["n_kmer_hits"], max(per_q)))
