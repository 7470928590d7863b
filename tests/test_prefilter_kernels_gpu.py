"""Kernel-level parity of the k-mer prefilter (uc_kmer_match.hip, uc_kmer_filter.hip, uc_diag_select.hip, uc_hit_lists.hip and the driver uc_prefilter.hip, stages E1-E4) on repeats, ties and window edges: Engine.prefilter() against the
oracle's E1-E4 run one query at a time with its stage counters, and - for homopolymers - against the closed form of spec UC-1 in plain integers
(tests/prefilter_cases.py).  Per-query counts, target / score / diag of every hit in list order and the four stage counters must be EQUAL.  The
preconditions that make each case reach its code path are proven on the CPU in tests/test_prefilter_cases.py.

That these tests can fail was checked with three result-only mutations of the prefilter's kernels (then in uc_prefilter.hip) on a scratch copy (never committed):
  diag_long_kernel taking the largest tied diagonal forward and the smallest for the mirrored pair (the two tie keys swapped) -> window sweep, tandem
      repeats, chunked runs, merge settings, loaded filter and X residues red (the closed form names the (query, target, diag) records);
  diag_long_kernel forgetting the run length carried across a window -> the same and the longest-sequence case red;
  rank_flag_kernel comparing with <= instead of < -> exactly the three ties-at-the-cut cases red (the list of every one of the 45 copies starts with
      (255, target 0), whose key is the query's bare key field, and gains one entry).
The whole module takes ~7 s on an MI355X, oracle side included."""
import os
import subprocess
import sys

import numpy as np
import pytest

import prefilter_cases as PC
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


def _assert_equals_oracle(got, ref):
    cnt, hits, st = got
    for k in PC.COUNTERS:
        assert st[k] == ref["totals"][k], (k, st[k], ref["totals"][k])
    assert np.array_equal(cnt, ref["cnt"]), np.nonzero(cnt != ref["cnt"])[0][:10]
    rh = np.concatenate(ref["hits"]) if len(ref["hits"]) else np.zeros(0, hits.dtype)
    q = np.repeat(np.arange(len(cnt)), cnt)
    for mine, theirs in (("target", "t"), ("score", "score"), ("diag", "diag")):
        bad = np.nonzero(hits[mine] != rh[theirs])[0]
        assert len(bad) == 0, "%s differs at (query, target, diag): got %s, oracle %s" % (
            mine, [(int(q[i]), int(hits["target"][i]), int(hits["diag"][i]), int(hits["score"][i])) for i in bad[:8]],
            [(int(q[i]), int(rh["t"][i]), int(rh["diag"][i]), int(rh["score"][i])) for i in bad[:8]])


def _assert_equals_closed_form(got, O, lengths, opts):
    cnt, hits, st = got
    p = util.oracle_params(O, opts)
    _, span = PC.pattern_offsets(p)
    sdiag = int(p.S3[PC.HOM * 21 + PC.HOM])
    assert 6 * sdiag >= p.kmer_thr
    lists, n_hits, n_cand = PC.hom_closed_form(lengths, sdiag, span, p.min_diag_hits, p.min_ungapped, p.max_seqs)
    assert st["n_kmer_hits"] == n_hits and st["n_candidates"] == n_cand and st["n_prefilter_hits"] == sum(len(l) for l in lists)
    assert cnt.tolist() == [len(l) for l in lists]
    flat = [r for l in lists for r in l]
    got_l = list(zip(hits["target"].tolist(), hits["score"].tolist(), hits["diag"].tolist()))
    q = np.repeat(np.arange(len(cnt)), cnt)
    bad = [(int(q[i]), got_l[i], flat[i]) for i in range(len(flat)) if got_l[i] != flat[i]]
    assert not bad, "(query, got (target, score, diag), closed form): %s" % bad[:8]
    # the pair the other way round: (t, q) comes out as min(0, Lt - Lq) - minus the LARGEST tied diagonal of (q, t)
    d = {(int(a), int(t)): int(dg) for a, t, dg in zip(q, hits["target"], hits["diag"])}
    for (a, t), dg in d.items():
        assert d[(t, a)] == min(0, lengths[t] - lengths[a])


_DEFAULT_RUNS = {}


def _default_run(name, s3, opts):
    """the engine's run of a case under the default environment, once per session"""
    if (name, opts) not in _DEFAULT_RUNS:
        _DEFAULT_RUNS[(name, opts)] = PC.run_engine(s3, opts)
    return _DEFAULT_RUNS[(name, opts)]


# ---------------------------------------------------------------- 1: window sweep
@pytest.mark.parametrize("opts", PC.SWEEP_OPTS, ids=["min_diag_hits_1", "double_hit_filter"])
def test_window_sweep(O, opts):
    """homopolymers of lengths 10 .. 33 and 58 .. 89: groups of 1 .. 6400 keys with runs of 1 .. 80 and boundaries at every offset modulo 64 - groups
    inside a window, ending in the next one, and long ones (diag_long_kernel) whose runs cross several windows; every longer target ties nq diagonals"""
    s3 = PC.hom(PC.SWEEP_LENGTHS)
    got = _default_run("sweep", s3, opts)
    _assert_equals_closed_form(got, O, PC.SWEEP_LENGTHS, opts)
    _assert_equals_oracle(got, PC.oracle_prefilter(O, s3, opts, key="sweep"))


# ---------------------------------------------------------------- 2: extreme diagonals and field widths
@pytest.mark.parametrize("wide", [False, True], ids=["compact", "wide"])
@pytest.mark.parametrize("lmax,n", PC.EXTREME_SETS)
def test_extreme_diagonals_and_field_widths(O, lmax, n, wide):
    """dbits 7 / 8 and tbits 5 / 6 by one residue or one sequence more; the one-k-mer sequence against the longest takes diagonal -(lmax - 10), the
    most negative value of the biased field, and the pair the other way round ties diagonal 0 with every diagonal up to lmax - 10"""
    lengths = PC.extreme_lengths(lmax, n)
    opts = PC.SWEEP_OPTS[0]
    got = PC.run_engine(PC.hom(lengths), opts, {"UC_PREFILTER_WIDE": "1"} if wide else None)
    big = lengths.index(lmax)
    cnt, hits, _ = got
    off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    first = hits[off[0]:off[1]]
    assert first["diag"][first["target"] == big].tolist() == [-(lmax - 10)]
    _assert_equals_closed_form(got, O, lengths, opts)
    _assert_equals_oracle(got, PC.oracle_prefilter(O, PC.hom(lengths), opts, key=("extreme", lmax, n)))


# ---------------------------------------------------------------- 3: tandem repeats
def test_tandem_repeats(O):
    """periods 7 and 13: diagonals a multiple of the period apart hold equal or near-equal counts - several long competing runs inside one group"""
    s3 = PC.tandem_repeats()
    _assert_equals_oracle(_default_run("repeat", s3, PC.REPEAT_OPTS), PC.oracle_prefilter(O, s3, PC.REPEAT_OPTS, key="repeat"))


# ---------------------------------------------------------------- 4: the longest sequence
def test_longest_sequence(O, U):
    """two sequences of 65,535 residues sharing a block at opposite ends: diagonals +-65,495 (dbits = 17, the 16-bit position field of wide entries,
    the j <= 65535 guards, the bias of the diagonal field).  Prefilter only."""
    s3 = PC.longest_pair()
    ref = PC.oracle_prefilter(O, s3, PC.LONGEST_OPTS, key="longest")
    for env in (None, {"UC_PREFILTER_WIDE": "1"}):
        got = PC.run_engine(s3, PC.LONGEST_OPTS, env)
        _assert_equals_oracle(got, ref)
        assert {65495, -65495} <= set(got[1]["diag"].tolist())


def test_sequence_beyond_the_limit_is_refused(U):
    e = U.Engine("-c 0.8", verbosity=1)
    try:
        with pytest.raises(U.UcError) as err:
            e.set_db(np.array([0, 65536, 65576], np.uint64), np.zeros(65576, np.uint8), np.zeros(65576, np.uint8))
        assert err.value.code == U.UC_ERR_ARGS
        e.set_db(np.array([0, 65535, 65575], np.uint64), np.zeros(65575, np.uint8), np.zeros(65575, np.uint8))      # the limit itself is fine
    finally:
        e.close()


# ---------------------------------------------------------------- 5: ties at the cut
@pytest.mark.parametrize("max_seqs", [20, 1, 44])
def test_ties_at_the_cut(O, max_seqs):
    """45 exact copies: every candidate of a copy has the saturated score 255, so --max-seqs keeps the smallest target ids and nothing else decides"""
    s3, copies = PC.tied_copies()
    opts = "-c 0.8 --max-seqs %d" % max_seqs
    got = PC.run_engine(s3, opts)
    cnt, hits, _ = got
    off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    for q in copies:
        mine = hits[off[q]:off[q + 1]]
        assert mine["target"].tolist() == copies[:max_seqs] and (mine["score"] == 255).all() and (mine["diag"] == 0).all(), q
    _assert_equals_oracle(got, PC.oracle_prefilter(O, s3, opts, key="ties"))


# ---------------------------------------------------------------- 6: several exact batches, chunks, merges
def _families():
    return {"sweep_min_diag_hits_1": (PC.hom(PC.SWEEP_LENGTHS), PC.SWEEP_OPTS[0], PC.SWEEP_CHUNK_RES, "sweep"),
            "sweep_double_hit_filter": (PC.hom(PC.SWEEP_LENGTHS), PC.SWEEP_OPTS[1], PC.SWEEP_CHUNK_RES, "sweep"),
            "repeat": (PC.tandem_repeats(), PC.REPEAT_OPTS, PC.REPEAT_CHUNK_RES, "repeat")}


def _assert_same_run(got, base):
    assert np.array_equal(got[0], base[0]) and got[1].tobytes() == base[1].tobytes()
    for k in PC.COUNTERS:
        assert got[2][k] == base[2][k], (k, got[2][k], base[2][k])


@pytest.mark.parametrize("family,variant", [("sweep_min_diag_hits_1", "hit_cap_floor"), ("sweep_double_hit_filter", "hit_cap_floor"),
                                            ("repeat", "hit_cap_floor"), ("repeat", "drun_max")])
def test_batch_cuts_change_nothing(O, family, variant):
    """UC_HIT_CAP at its floor of 2^20 keys cuts the ~4-5 M hits into >= 4 exact batches per super-batch (cut_batch cuts on the per-query totals, which
    the CPU preconditions bound: total > 3 x 2^20, every query < 2^20); UC_DRUN_MAX=8 cuts the super-batch of the repeats, whose distinct k-mers
    have 19 runs (the homopolymers have ONE distinct k-mer with one run, which no budget can cut: they are not run under it).  Byte-identical hit
    arrays and the same counters as the default run, which equals the oracle."""
    s3, opts, _, key = _families()[family]
    base = _default_run(key, s3, opts)
    _assert_equals_oracle(base, PC.oracle_prefilter(O, s3, opts, key=key))
    _assert_same_run(PC.run_engine(s3, opts, {"UC_HIT_CAP": "1048576"} if variant == "hit_cap_floor" else {"UC_DRUN_MAX": "8"}), base)


@pytest.mark.parametrize("family", ["sweep_min_diag_hits_1", "sweep_double_hit_filter", "repeat"])
def test_target_chunks_symmetric_and_full_grid(O, family):
    """>= 3 target chunks, walked as the upper triangle with the pairs the other way round mirrored (minus the LARGEST tied diagonal: on the
    homopolymers this is where the mirrored tie-break meets real ties) and as the full grid.  The triangle is really taken: same n_kmer_hits as the
    oracle from fewer expanded keys than the full grid."""
    s3, opts, chunk, key = _families()[family]
    base = _default_run(key, s3, opts)
    ref = PC.oracle_prefilter(O, s3, opts, key=key)
    sym = PC.run_engine(s3, opts, {"UC_PREFILTER_CHUNK_RES": chunk})
    full = PC.run_engine(s3, opts, {"UC_PREFILTER_CHUNK_RES": chunk, "UC_PREFILTER_SYMMETRIC": "0"})
    _assert_equals_oracle(sym, ref)
    _assert_equals_oracle(full, ref)
    _assert_same_run(sym, base)
    _assert_same_run(full, base)
    assert sym[2]["n_kmer_hits"] == ref["totals"]["n_kmer_hits"]
    # fewer keys reach the sort under the triangle than under the full grid: this also shows that the chunks survived the engine's density re-cut (one
    # chunk would make the two runs the same run)
    if "--min-diag-hits 1" in opts:      # (n_filtered_hits counts the keys that reach the sort: all expanded keys without the filter, its survivors with it)
        assert sym[2]["n_filtered_hits"] < full[2]["n_filtered_hits"] == ref["totals"]["n_kmer_hits"]
    else:
        assert sym[2]["n_filtered_hits"] < full[2]["n_filtered_hits"]


def test_merge_sorted_in_both_settings(O, tmp_path):
    """the chunk accumulator merged with every pass's list as two sorted runs (default) or re-sorted with it (UC_MERGE_SORTED=0): the setting is read
    once per process, so each runs in a child; same arrays as the oracle's"""
    outs = []
    for tag, extra in (("merge", {"UC_MERGE_SORTED": "1"}), ("sort", {"UC_MERGE_SORTED": "0"})):
        path = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(util.ROOT, "tests", "prefilter_cases.py"), path], env=dict(os.environ, **extra),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(np.load(path))
    for name, key, s3, opts in (("sweep", "sweep", PC.hom(PC.SWEEP_LENGTHS), PC.SWEEP_OPTS[0]), ("sweep_filter", "sweep", PC.hom(PC.SWEEP_LENGTHS), PC.SWEEP_OPTS[1]),
                                ("repeat", "repeat", PC.tandem_repeats(), PC.REPEAT_OPTS)):
        ref = PC.oracle_prefilter(O, s3, opts, key=key)
        for o in outs:
            st = dict(zip(PC.COUNTERS, (int(x) for x in o[name + "_counters"][:4])))
            _assert_equals_oracle((o[name + "_cnt"], o[name + "_hits"], st), ref)
        assert outs[0][name + "_hits"].tobytes() == outs[1][name + "_hits"].tobytes()


# ---------------------------------------------------------------- 7: a loaded filter
def test_loaded_filter(O):
    """60 targets of 400 residues and one query of 2,000 over the three letters with the largest diagonal score: 14,877,437 k-mer hits, the long
    query alone 1,159,810 in 33,358 runs (17 tiles of 2048 runs in filter_kernel), nearly every key a multiple hit; the oracle takes ~1.7 s on 8
    threads.  The region, the survivor area, level 2 and the key sort run at full volume.  (60 targets x 2,400 diagonals bound the long query's
    distinct keys by 144,000: bitmap saturation is test_saturating_filter's.)"""
    s3 = PC.loaded_filter(O)
    ref = PC.oracle_prefilter(O, s3, PC.LOADED_OPTS, key="loaded")
    got = PC.run_engine(s3, PC.LOADED_OPTS)
    _assert_equals_oracle(got, ref)
    print("loaded filter: %d of %d keys survive the double-hit filter" % (got[2]["n_filtered_hits"], got[2]["n_kmer_hits"]))


def test_saturating_filter(O):
    """1,400 random targets of 80 residues and one query of 2,000 over the five letters with the largest diagonal score: the long query's 744,905
    k-mer hits fall on 572,116 distinct (target, diagonal) keys, more than the 2^19 bits of either LDS bitmap of filter_kernel - both levels run
    saturated, nearly everything survives them and only the exact count after the sort separates single from double hits.  38,023,899 hits and
    1,817,093 candidates in the whole case; the oracle takes 2.7 s on 8 threads."""
    s3 = PC.saturating_filter(O)
    ref = PC.oracle_prefilter(O, s3, PC.SATURATING_OPTS, key="saturating")
    got = PC.run_engine(s3, PC.SATURATING_OPTS)
    _assert_equals_oracle(got, ref)
    print("saturating filter: %d of %d keys survive the double-hit filter" % (got[2]["n_filtered_hits"], got[2]["n_kmer_hits"]))


# ---------------------------------------------------------------- 8: X residues
@pytest.mark.parametrize("name", ["x_hom", "x_rep"])
def test_x_residues(O, name):
    """an X at position 0, at the last k-mer's last letter, at every 10th residue and on residues 0, 4, 8 of every ten (no valid k-mer left): the
    last kind is nobody's target and has no list; the others are found and scored across their X residues"""
    s3, variant, opts = PC.x_cases()[name]
    got = PC.run_engine(s3, opts)
    _assert_equals_oracle(got, PC.oracle_prefilter(O, s3, opts, key=name))
    cnt, hits, _ = got
    dead = [i for i, v in enumerate(variant) if v == "x_none_valid"]
    assert dead and not np.isin(hits["target"], dead).any() and cnt[dead].sum() == 0
    assert all(cnt[i] > 0 for i, v in enumerate(variant) if v != "x_none_valid")
