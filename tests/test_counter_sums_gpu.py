"""The counters that the streaming kernels sum per workgroup (block_add, uc_device.h): every figure equals the sum computed in
numpy or by the oracle, on 1 workgroup, on 3 and on the default grid (UC_COUNT_GRID_CAP = 1, 3, unset; read once per engine).  The list sizes
cover a partial wave, a partial workgroup and a grid-stride loop that wraps while other workgroups get nothing."""
import os

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
CAPS = (None, 1, 3)
SIZES = (1, 63, 64, 65, 255, 256, 257, 769, 1025)
# 2040 x 3000 = 6,120,000 cells: 900 such pairs sum past 2^32 (queries stay in the single-strip classes, SW_MAX_ROWS = 2048)
LENGTHS = (2040, 3000, 1900, 2048, 300, 35, 1)


def _engine(cap, opts="-c 0.8"):
    import unicore_amd as U
    old = os.environ.pop("UC_COUNT_GRID_CAP", None)
    if cap is not None:
        os.environ["UC_COUNT_GRID_CAP"] = str(cap)
    try:
        return U.Engine(opts, verbosity=1)
    finally:
        os.environ.pop("UC_COUNT_GRID_CAP", None)
        if old is not None:
            os.environ["UC_COUNT_GRID_CAP"] = old


@pytest.fixture(scope="module")
def db():
    rng = np.random.default_rng(412)
    s3 = [rng.integers(0, 20, L, dtype=np.uint8) for L in LENGTHS]
    sa = [rng.integers(0, 20, L, dtype=np.uint8) for L in LENGTHS]
    return dict(s3=s3, sa=sa, len=np.array(LENGTHS, np.int64), flat=util.flat(s3, sa))


@pytest.fixture(scope="module")
def engines(db):
    out = {}
    for cap in CAPS:
        e = _engine(cap)
        e.set_db(*db["flat"])
        out[cap] = e
    return out


def _pairs(n, seed):
    """mostly the two longest sequences (the 64-bit sum), the rest anything"""
    rng = np.random.default_rng(seed)
    q, t = rng.integers(0, len(LENGTHS), n), rng.integers(0, len(LENGTHS), n)
    big = rng.random(n) < 0.9
    q[big], t[big] = 0, 1
    return q.astype(np.uint32), t.astype(np.uint32)


@pytest.mark.parametrize("n", SIZES)
def test_forward_pass_cells_and_bytes(db, engines, n):
    """plan_key_kernel: cells_run and sw_algorithmic_bytes of one MODE 0 pass (int32 table: nothing is run twice)"""
    q, t = _pairs(n, 1000 + n)
    lq, lt = db["len"][q], db["len"][t]
    cells, alg = int((lq * lt).sum()), int((2 * (lq + lt) + 32).sum())
    if n == 1025:
        assert cells > 1 << 32
    scores = None
    for cap in CAPS:
        e = engines[cap]
        e.reset_stats()
        r = e.sw_pass(0, 0, q, t)
        st = e.stats()
        print("n %d cap %s: cells_run %d (numpy %d), sw_algorithmic_bytes %d (numpy %d)" % (n, cap, st["cells_run"], cells, st["sw_algorithmic_bytes"], alg))
        assert st["cells_run"] == cells, cap
        assert st["sw_algorithmic_bytes"] == alg, cap
        if scores is None:
            scores = r["score"]
        assert np.array_equal(r["score"], scores), cap


def _candidates(db, n, seed):
    rng = np.random.default_rng(seed)
    q, t = rng.integers(0, len(LENGTHS), n), rng.integers(0, len(LENGTHS), n)
    same = rng.random(n) < 0.3          # a sequence against itself near the main diagonal: scores above any threshold
    t[same] = q[same]
    lq, lt = db["len"][q], db["len"][t]
    diag = rng.integers(-(lt - 1), np.maximum(lq, 1))
    diag[same] = rng.integers(-2, 3, int(same.sum()))
    diag = np.clip(diag, -(lt - 1), lq - 1)
    return q, t, diag


def _overlap(db, q, t, diag):
    lq, lt = db["len"][q], db["len"][t]
    return np.maximum(np.minimum(lq, lt + diag) - np.maximum(diag, 0), 0)


@pytest.mark.parametrize("n", SIZES)
def test_ungapped_bytes_and_kept_count(db, engines, n):
    """ungapped_kernel's overlap sum (the stage's algorithmic bytes are overlap + 16 per candidate) and select_key_kernel's kept count"""
    q, t, diag = _candidates(db, n, 2000 + n)
    ovl = int(_overlap(db, q, t, diag).sum())
    min_score = 30
    ref = engines[None].ungapped(q, t, diag)
    kept = int((ref >= min_score).sum())
    if n >= 63:
        assert 0 < kept < n
    for cap in CAPS:
        s, got_ovl, got_kept = engines[cap].ungapped_select(q, t, diag, min_score)
        print("n %d cap %s: overlap %d (numpy %d), bytes %d, kept %d (numpy %d)" % (n, cap, got_ovl, ovl, got_ovl + 16 * n, got_kept, kept))
        assert np.array_equal(s, ref), cap
        assert got_ovl == ovl, cap
        assert got_kept == kept, cap


@pytest.mark.parametrize("n", (1, 65, 257, 1025))
def test_all_zero_contributions_leave_the_counters_at_zero(db, engines, n):
    """diagonals that miss the target altogether: no overlap, score 0, nothing kept - no workgroup issues its atomic"""
    rng = np.random.default_rng(3000 + n)
    q, t = rng.integers(0, len(LENGTHS), n), rng.integers(0, len(LENGTHS), n)
    diag = db["len"][q] + rng.integers(0, 5, n)
    assert not _overlap(db, q, t, diag).any()
    for cap in CAPS:
        s, ovl, kept = engines[cap].ungapped_select(q, t, diag, 1)
        assert not s.any() and ovl == 0 and kept == 0, cap


@pytest.fixture(scope="module")
def golden_ref():
    from oracle import oracle_py as O
    opts = str(np.load(os.path.join(GOLD, "expected_default.npz"))["options"])
    ref = O.cluster(O.OracleDb(os.path.join(GOLD, "db")), util.oracle_params(O, opts), threads=8)
    return opts, ref["counts"]


def test_diagonal_selection_on_one_and_three_workgroups(monkeypatch):
    """diag_select_kernel runs under the same grid cap (every wave ends on one atomic on the candidate cursor).  Every query through the batch sort
    (UC_TD_ONCHIP=0), 1,842 candidates: on 1 workgroup each of its four waves drains its 64-candidate stage several times before its last, partial one.
    Candidates and hit lists stay the oracle's (order of the appends does not matter: E4 sorts on a unique key)"""
    from oracle import oracle_py as O
    monkeypatch.setenv("UC_TD_ONCHIP", "0")
    s3, sa = util.family_db(29, n_fam=30, members=8)
    ref = O.cluster(O.OracleDb(s3=s3, sa=sa), util.oracle_params(O, "-c 0.8"), threads=8)
    cnt = ref["hit_cnt"]
    rh = np.concatenate([ref["hits"][i, : cnt[i]] for i in range(len(cnt))])
    assert ref["counts"]["n_candidates"] > 4 * 64 * 4
    for cap in CAPS:
        e = _engine(cap)
        e.set_db(*util.flat(s3, sa))
        e.prefilter()
        st = e.stats()
        got_cnt, hits = e.hits()
        print("cap %s: n_candidates %d (oracle %d), td_onchip_queries %d" % (cap, st["n_candidates"], ref["counts"]["n_candidates"], st["td_onchip_queries"]))
        assert st["td_onchip_queries"] == 0
        for k in ("n_candidates", "n_sim_kmers", "n_kmer_hits", "n_prefilter_hits"):
            assert st[k] == ref["counts"][k], (cap, k)
        assert np.array_equal(got_cnt, cnt), cap
        for f, g in (("target", "t"), ("score", "score"), ("diag", "diag")):
            assert np.array_equal(hits[f], rh[g]), (cap, f)
        e.close()


def test_pipeline_counters_equal_the_oracle(golden_ref):
    """align() on the small golden database: cells_fwd / cells_rev / cells_start (cells_kernel, cells_box_kernel) and the prefilter's
    n_sim_kmers (position_runs_kernel) equal the oracle's; every other counter is the same on 1 workgroup as on the default grid"""
    opts, c = golden_ref
    figures = {}
    for cap in CAPS:
        e = _engine(cap, opts)
        e.load_db(os.path.join(GOLD, "db"))
        e.prefilter()
        e.align()
        st = e.stats()
        print("cap %s: %s" % (cap, {k: st[k] for k in ("cells_fwd", "cells_rev", "cells_start", "cells_run", "sw_algorithmic_bytes", "n_sim_kmers")}))
        for a, b in (("cells_fwd", "cells_fwd"), ("cells_rev", "cells_rev"), ("cells_start", "cells_start"), ("n_sim_kmers", "n_sim_kmers"),
                     ("n_candidates", "n_candidates"), ("n_prefilter_hits", "n_prefilter_hits"), ("n_gapped_alignments", "n_alignments")):
            assert st[a] == c[b], (cap, a, st[a], c[b])
        assert st["cells_fwd"] > 0 and st["cells_rev"] > 0 and st["cells_start"] > 0
        figures[cap] = {k: v for k, v in st.items() if isinstance(v, int)} | {"algorithmic_bytes": list(st["algorithmic_bytes"])}
        e.close()
    assert figures[1] == figures[None]
    assert figures[3] == figures[None]


def test_traceback_cells_do_not_depend_on_the_grid():
    """cells_tb_kernel (the traceback boxes, --min-seq-id): the same sum on 1 and 3 workgroups as on the default grid, records unchanged"""
    figures, recs = {}, {}
    for cap in CAPS:
        e = _engine(cap, "-c 0.5 --min-seq-id 0.3")
        e.load_db(os.path.join(GOLD, "db"))
        e.prefilter()
        e.align()
        st = e.stats()
        print("cap %s: cells_tb %d" % (cap, st["cells_tb"]))
        figures[cap] = {k: v for k, v in st.items() if isinstance(v, int)}
        recs[cap] = e.alns().tobytes()
        e.close()
    assert figures[None]["cells_tb"] > 0
    assert figures[1] == figures[None] and figures[3] == figures[None]
    assert recs[1] == recs[None] and recs[3] == recs[None]
