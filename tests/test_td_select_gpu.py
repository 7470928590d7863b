"""The on-chip diagonal selection of the k-mer prefilter (td_select_kernel / cand_gather_kernel, uc_diag_select.hip) against the batch sort it replaces
and against the oracle.  Every case compares three runs of Engine.prefilter(): the default one, the one with UC_TD_ONCHIP=0 (every query through
compact_kernel, the radix sort, diag_select_kernel and diag_long_kernel) and the oracle's E1-E4 - or the closed form of spec UC-1 where one exists.
Per-query counts, target / score / diag of every hit in list order and the stage counters, n_filtered_hits included, must be EQUAL.

A homopolymer query of nq k-mer positions against a target of nt has hom_cnt(nq, nt, d) hits on diagonal d, and the double-hit filter keeps exactly
the hits of the diagonals with at least two: the survivor count of every query is computed here from PC.hom_cnt and checked against the engine's
n_filtered_hits (a false positive of the filter's bitmaps would show there), so the cases below KNOW on which side of the cap every query falls.
That td_select_kernel really took them is read from the engine (stats: td_onchip_queries / td_onchip_keys) and asserted wherever the share is known."""
import numpy as np
import pytest

import prefilter_cases as PC
import test_prefilter_kernels_gpu as TK
import util

pytestmark = pytest.mark.gpu

OFF = {"UC_TD_ONCHIP": "0"}
FILTERED = PC.COUNTERS + ("n_filtered_hits",)
THREADS, CLASSES = 256, (1, 2, 4, 8, 16, 32)       # td_select_kernel: threads per workgroup and the items-per-thread instantiations; the default cap is 8192


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _span(O, opts):
    return PC.pattern_offsets(util.oracle_params(O, opts))[1]


def _same(got, base):
    """byte-identical lists and the same counters, the keys that reach the selection included"""
    assert np.array_equal(got[0], base[0]) and got[1].tobytes() == base[1].tobytes()
    for k in FILTERED:
        assert got[2][k] == base[2][k], (k, got[2][k], base[2][k])


def _both(s3, opts, env=None):
    """-> (default run, UC_TD_ONCHIP=0 run) under `env`, asserted equal; the second took nothing on chip"""
    on = PC.run_engine(s3, opts, dict(env or {}))
    off = PC.run_engine(s3, opts, dict(env or {}, **OFF))
    _same(on, off)
    assert off[2]["td_onchip_queries"] == 0 and off[2]["td_onchip_keys"] == 0
    return on, off


def _taken(st):
    return st["td_onchip_queries"], st["td_onchip_keys"]


def _all_on_chip(st):
    """every surviving key of the run went through td_select_kernel: no query had more survivors than the cap"""
    assert 0 < st["td_onchip_keys"] == st["n_filtered_hits"], (st["td_onchip_keys"], st["n_filtered_hits"])


def hom_survivors(groups, span):
    """groups: [(letter, lengths)] of homopolymers whose letters' k-mers are similar to themselves only -> survivors of the double-hit filter per query in
    database order: the hits on the diagonals that hold at least two"""
    out = []
    for _, lengths in groups:
        for Lq in lengths:
            nq, n = Lq - span + 1, 0
            for Lt in lengths:
                nt = Lt - span + 1
                if nq >= 1 and nt >= 1:
                    n += sum(c for c in (PC.hom_cnt(nq, nt, d) for d in range(-(nt - 1), nq)) if c >= 2)
            out.append(n)
    return out


# ---------------------------------------------------------------- the cap edge
# k-mer positions per sequence and letter: with T the targets of the letter that hold >= 2 positions a query keeps nq * sum(T) - 2 |T| keys, which gives
# 63 / 64 / 65 and 255 / 256 / 257 survivors to the first sequence of groups 1-3 and 4-6 (the second of group 1 and of group 5) - computed and asserted below
EDGE_GROUPS = ((2, (2, 3, 18, 1)), (3, (2, 32)), (4, (3, 20)), (5, (7, 30)), (6, (7, 13)), (7, (9, 20)))


@pytest.mark.parametrize("cap", [64, 256])
def test_cap_edge(O, cap):
    """queries with exactly cap - 1, cap and cap + 1 survivors in one batch, next to one with a single k-mer (no survivor: the n == 0 branch) and to
    queries far above the cap: both paths and the hand-over in one call"""
    opts = PC.SWEEP_OPTS[1]
    span = _span(O, opts)
    p = util.oracle_params(O, opts)
    groups = [(a, [n + span - 1 for n in pos]) for a, pos in EDGE_GROUPS]
    letters = [a for a, _ in groups]
    assert all(6 * p.S3[a * 21 + a] >= p.kmer_thr for a in letters) and all(6 * p.S3[a * 21 + b] < p.kmer_thr for a in letters for b in letters if a != b)
    s3 = [x for a, lengths in groups for x in PC.hom(lengths, a)]
    surv = hom_survivors(groups, span)
    assert {cap - 1, cap, cap + 1} <= set(surv) and 0 in surv and max(surv) > cap + 1, surv
    on, off = _both(s3, opts, {"UC_TD_ONCHIP_CAP": str(cap)})
    assert on[2]["n_filtered_hits"] == sum(surv)
    assert _taken(on[2]) == (sum(1 for n in surv if 0 < n <= cap), sum(n for n in surv if n <= cap))
    TK._assert_equals_oracle(on, PC.oracle_prefilter(O, s3, opts, key="td_edge"))


# ---------------------------------------------------------------- items-per-thread classes
CLASS_POSITIONS = (2, 3, 6, 12, 24, 48)


def test_every_items_per_thread_class(O):
    """one letter, six lengths: the survivor counts 178, 273, 558, 1128, 2268 and 4548 fall into the six instantiations below the default cap"""
    opts = PC.SWEEP_OPTS[1]
    span = _span(O, opts)
    lengths = [n + span - 1 for n in CLASS_POSITIONS]
    surv = hom_survivors([(PC.HOM, lengths)], span)
    hit = {min(c for c in CLASSES if n <= c * THREADS) for n in surv if 0 < n <= CLASSES[-1] * THREADS}
    assert hit == set(CLASSES), surv
    on, off = _both(PC.hom(lengths), opts)
    assert on[2]["n_filtered_hits"] == sum(surv) and _taken(on[2]) == (len(surv), sum(surv))
    TK._assert_equals_closed_form(on, O, lengths, opts)
    TK._assert_equals_oracle(on, PC.oracle_prefilter(O, PC.hom(lengths), opts, key="td_classes"))


# ---------------------------------------------------------------- ties and long runs
def small_repeats(seed=17):
    """three sequences of period 13 (60, 70, 80 residues) and three of period 7 (40, 50, 64), each over one random unit and starting at its own phase: a
    query hits every same-phase position of its period's sequences, ~n x 180 / 13 keys at most - far below the cap, unlike PC.tandem_repeats()"""
    rng = np.random.default_rng(seed)
    s3 = []
    for period, lengths in ((13, (60, 70, 80)), (7, (40, 50, 64))):
        unit = rng.integers(0, 20, period, dtype=np.uint8)
        for k, L in enumerate(lengths):
            s3.append(np.tile(unit, L // period + 3)[k: k + L].copy())
    return s3


def test_small_tandem_repeats_on_chip(O):
    """diagonals a period apart hold equal counts inside one group - the smallest must win, and for the pair the other way round the largest - with every
    query of the case on chip (asserted from the engine's count); with and without the mirrored passes of a chunked run"""
    s3 = small_repeats()
    ref = PC.oracle_prefilter(O, s3, PC.REPEAT_OPTS, key="td_small_repeats")
    on, _ = _both(s3, PC.REPEAT_OPTS)
    _all_on_chip(on[2])
    assert on[2]["td_onchip_queries"] == len(s3)
    TK._assert_equals_oracle(on, ref)
    # a tie is really there: some listed pair has a second diagonal with the count of the chosen one
    offs, span = PC.pattern_offsets(util.oracle_params(O, PC.REPEAT_OPTS))
    cnt, hits, _st = on
    q = np.repeat(np.arange(len(cnt)), cnt)
    ties = 0
    for a, t, d in zip(q.tolist(), hits["target"].tolist(), hits["diag"].tolist()):
        c = PC.exact_diagonal_counts(s3[a], s3[t], offs, span)
        ties += sum(1 for v in c.values() if v == max(c.values())) > 1 and d == min(k for k, v in c.items() if v == max(c.values()))
    assert ties > 0
    chunked, _ = _both(s3, PC.REPEAT_OPTS, {"UC_PREFILTER_CHUNK_RES": "120"})
    TK._assert_same_run(chunked, on)          # (the triangle expands fewer keys: n_filtered_hits differs from the unchunked run's)
    assert chunked[2]["td_onchip_keys"] == chunked[2]["n_filtered_hits"] > 0


LONG_RUN_LENGTHS = (120, 2300, 5000)


def test_runs_across_waves(O):
    """three unrelated random sequences: each hits itself on diagonal 0 as ONE run - a key for every k-mer that is similar to itself, ~97 % of the
    positions - and next to nothing else, so runs of ~111, ~2,200 and ~4,900 keys are sorted at 1, 16 and 32 keys per thread and lie across two or
    more waves of the sorted array (64 threads each): scan A, the carried run start and the keys at the thread edges decide the count.  The classes are
    asserted: the self-hits are a lower bound of a query's survivors, all its k-mer hits (the oracle's count per query) an upper one."""
    rng = np.random.default_rng(23)
    s3 = [rng.integers(0, 20, L, dtype=np.uint8) for L in LONG_RUN_LENGTHS]
    ref = PC.oracle_prefilter(O, s3, PC.REPEAT_OPTS, key="td_long_runs")
    p = ref["params"]
    offs, span = PC.pattern_offsets(p)
    runs = [sum(1 for i in range(len(x) - span + 1) if sum(int(p.S3[int(x[i + o]) * 21 + int(x[i + o])]) for o in offs) >= p.kmer_thr) for x in s3]
    hits_q = [c["n_kmer_hits"] for c in ref["per_query"]]
    for run, h, lo, hi in zip(runs, hits_q, (64, 8 * THREADS, 16 * THREADS), (1 * THREADS, 16 * THREADS, 32 * THREADS)):
        assert lo < run <= h <= hi, (runs, hits_q)
    assert runs[1] > 64 * 16 and runs[2] > 64 * 32          # more than a wave's keys in one run at 16 and at 32 keys per thread
    on, _ = _both(s3, PC.REPEAT_OPTS)
    _all_on_chip(on[2])
    assert on[2]["td_onchip_queries"] == 3 and on[2]["n_filtered_hits"] >= sum(runs)
    cnt, hits, _st = on
    off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    for a in range(3):
        mine = hits[off[a]:off[a + 1]]
        assert mine["diag"][mine["target"] == a].tolist() == [0], a
    TK._assert_equals_oracle(on, ref)


@pytest.mark.parametrize("cap", [None, "1024"])
def test_tandem_repeats(O, cap):
    """PC.tandem_repeats(): every query keeps tens of thousands of keys, above any cap - the whole case takes the batch sort behind td_select_kernel's
    n > cap branch (nothing is taken on chip: asserted), which must leave regions and counts as it found them"""
    s3 = PC.tandem_repeats()
    on, _ = _both(s3, PC.REPEAT_OPTS, {"UC_TD_ONCHIP_CAP": cap} if cap else None)
    assert _taken(on[2]) == (0, 0)
    TK._assert_equals_oracle(on, PC.oracle_prefilter(O, s3, PC.REPEAT_OPTS, key="repeat"))


@pytest.mark.parametrize("max_seqs", [1, 20, 44])
def test_tied_copies(O, max_seqs):
    s3, copies = PC.tied_copies()
    opts = "-c 0.8 --max-seqs %d" % max_seqs
    on, _ = _both(s3, opts)
    cnt, hits, _st = on
    off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    for q in copies:
        mine = hits[off[q]:off[q + 1]]
        assert mine["target"].tolist() == copies[:max_seqs] and (mine["diag"] == 0).all(), q
    TK._assert_equals_oracle(on, PC.oracle_prefilter(O, s3, opts, key="ties"))


# ---------------------------------------------------------------- collision survivors
@pytest.mark.parametrize("case", ["loaded", "saturating"])
def test_collision_survivors(O, case):
    """most survivors of these filters are single hits that the exact count must drop again; the 2,000-residue query exceeds every cap and takes the
    batch sort, under the default cap and under a lower one that hands more of the short sequences over with it"""
    s3, opts = (PC.loaded_filter(O), PC.LOADED_OPTS) if case == "loaded" else (PC.saturating_filter(O), PC.SATURATING_OPTS)
    ref = PC.oracle_prefilter(O, s3, opts, key=case)
    on, _ = _both(s3, opts)
    TK._assert_equals_oracle(on, ref)
    low = PC.run_engine(s3, opts, {"UC_TD_ONCHIP_CAP": "2048"})
    _same(low, on)


# ---------------------------------------------------------------- mirrored passes
@pytest.mark.parametrize("symmetric", [True, False], ids=["triangle", "full_grid"])
@pytest.mark.parametrize("family", ["sweep_min_diag_hits_1", "sweep_double_hit_filter", "repeat"])
def test_target_chunks(O, family, symmetric):
    """>= 3 target chunks: under the triangle the groups of the queries behind the chunk also yield the pair the other way round, which takes the LARGEST
    tied diagonal (on the homopolymers every longer target ties) - on chip as in diag_select_kernel"""
    s3, opts, chunk, key = TK._families()[family]
    env = {"UC_PREFILTER_CHUNK_RES": chunk}
    if not symmetric:
        env["UC_PREFILTER_SYMMETRIC"] = "0"
    on, _ = _both(s3, opts, env)
    if key == "sweep":
        TK._assert_equals_closed_form(on, O, PC.SWEEP_LENGTHS, opts)
    TK._assert_equals_oracle(on, PC.oracle_prefilter(O, s3, opts, key=key))


# ---------------------------------------------------------------- several exact batches
@pytest.mark.parametrize("opts", PC.SWEEP_OPTS, ids=["min_diag_hits_1", "double_hit_filter"])
def test_several_exact_batches(O, opts):
    """UC_HIT_CAP at its floor: several exact batches per super-batch, so the per-batch candidate offsets and the reuse of the regions are exercised"""
    s3 = PC.hom(PC.SWEEP_LENGTHS)
    on, _ = _both(s3, opts, {"UC_HIT_CAP": "1048576"})
    TK._assert_equals_closed_form(on, O, PC.SWEEP_LENGTHS, opts)
    TK._assert_equals_oracle(on, PC.oracle_prefilter(O, s3, opts, key="sweep"))


# ---------------------------------------------------------------- several exact batches and mirrored passes with every query on chip
MANY_POSITIONS = (20,) * 19 + (12, 5, 3, 2)


def _many_short(O, opts):
    """every letter whose k-mer is similar to itself only, 23 homopolymers each (19 of 20 k-mer positions): at most 20 x 402 - 46 = 7,994 survivors per
    query, ~161,600 hits per letter -> (sequences, survivors per query)"""
    p = util.oracle_params(O, opts)
    span = _span(O, opts)
    good = [a for a in range(20) if 6 * p.S3[a * 21 + a] >= p.kmer_thr]
    letters = [a for a in good if all(6 * p.S3[a * 21 + b] < p.kmer_thr for b in good if b != a)]
    groups = [(a, [n + span - 1 for n in MANY_POSITIONS]) for a in letters]
    return [x for a, lengths in groups for x in PC.hom(lengths, a)], hom_survivors(groups, span)


def test_several_exact_batches_on_chip(O):
    """more than 2 x 2^20 k-mer hits under UC_HIT_CAP at its floor: at least three exact batches, every one of them with region-resident records, so
    the per-batch candidate offsets and the reuse of the regions are the on-chip path's"""
    opts = PC.SWEEP_OPTS[1]
    s3, surv = _many_short(O, opts)
    assert max(surv) <= CLASSES[-1] * THREADS
    on, _ = _both(s3, opts, {"UC_HIT_CAP": "1048576"})
    assert on[2]["n_kmer_hits"] > 2 << 20
    assert on[2]["n_filtered_hits"] == sum(surv) and _taken(on[2]) == (len(surv), sum(surv))
    _same(PC.run_engine(s3, opts), on)
    TK._assert_equals_oracle(on, PC.oracle_prefilter(O, s3, opts, key="td_many"))


@pytest.mark.parametrize("symmetric", [True, False], ids=["triangle", "full_grid"])
def test_target_chunks_on_chip(O, symmetric):
    """the same database in chunks of < 400 target positions: every query of every pass is on chip, the mirrored ones (queries behind the chunk, every
    longer target tying its diagonals) included"""
    opts = PC.SWEEP_OPTS[1]
    s3, surv = _many_short(O, opts)
    env = {"UC_PREFILTER_CHUNK_RES": PC.SWEEP_CHUNK_RES}
    if not symmetric:
        env["UC_PREFILTER_SYMMETRIC"] = "0"
    on, _ = _both(s3, opts, env)
    _all_on_chip(on[2])
    if not symmetric:
        assert on[2]["n_filtered_hits"] == sum(surv)
    else:
        assert on[2]["n_filtered_hits"] < sum(surv)
    TK._assert_equals_oracle(on, PC.oracle_prefilter(O, s3, opts, key="td_many"))


# ---------------------------------------------------------------- wide mode
@pytest.mark.parametrize("lmax,n", PC.EXTREME_SETS)
def test_wide_mode(O, lmax, n):
    """UC_PREFILTER_WIDE=1 keeps the u64 regions and with them the batch sort for every query: equal results in both settings of the switch"""
    lengths = PC.extreme_lengths(lmax, n)
    opts = PC.SWEEP_OPTS[1]
    on, _ = _both(PC.hom(lengths), opts, {"UC_PREFILTER_WIDE": "1"})
    assert _taken(on[2]) == (0, 0)
    _same(PC.run_engine(PC.hom(lengths), opts), on)
    TK._assert_equals_closed_form(on, O, lengths, opts)
    TK._assert_equals_oracle(on, PC.oracle_prefilter(O, PC.hom(lengths), opts, key=("td_extreme", lmax, n)))
