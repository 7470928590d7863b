"""Kernel-level tests of the gapped stage (E5/E6): every length class of every class table in every mode it runs, one pass at a time
(uc_engine_sw_pass), against the scalar oracle - exact integer comparisons.  Engine.align only reaches the classes and modes its prefilter
happens to produce; here the pair lists are built for them: queries at both edges and the middle of every class, related targets (mutated
copies with indels, shifted starts, truncated copies, copies whose first or last residue pair scores 0 - several optimal rows) and
unrelated ones (1, 2, 63, 64, 65 residues, the query's length, longer than 2048), an odd pair count per query (a slot that runs with its
first pair only) and queries with more pairs than a task holds."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import util
from sw_dp import Dp

pytestmark = pytest.mark.gpu

# the class tables of uc_sw_plan.hip (h_tab): row caps and pairs per workgroup task.  The library reports the class of every pair; the sweep
# asserts it equals the one computed from these lists, so a change to either side shows up here.
CAPS = {0: [64, 128, 192, 256, 320, 384, 448, 512, 640, 768, 896, 1024, 1280, 1536, 1792, 2048],
        1: [32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 448, 512, 576, 640, 704, 768, 896, 1024, 1152, 1280, 1408, 1536,
            1664, 1792, 1920, 2048],
        2: [64, 128, 192, 256, 384, 512, 768, 1024, 1280, 1536, 1792, 2048],
        3: [128, 256, 384, 512, 640, 768, 896, 1024, 1152, 1280, 1408, 1536, 1664, 1792, 1920, 2048]}
TCAP = {0: [256] * 8 + [64] * 4 + [24] * 4, 1: [64] * 18 + [48] * 6 + [24] * 4, 2: [256] * 4 + [64] * 2 + [24] * 6,
        3: [8] * 6 + [16] * 10}
MODES = {0: (0, 1, 2), 1: (0, 1, 2, 4, 6, 7), 2: (3,), 3: (4, 6)}
LONG_TASK = 8                  # SW_LONG_TASK_PAIRS: pairs per task of the long-query kernel
SW_PK_OVF = 0x7C00 - 256       # packed scores at or above this are re-run in int32
TE_UNIQUE = 1 << 30            # SW_TE_UNIQUE: MODE 6 found every optimal cell in one row
BANDS = (0, 1, 4, 48)


def class_of(L, tab):
    c = 0
    while c < len(CAPS[tab]) and CAPS[tab][c] < L:
        c += 1
    return c


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _pmap(fn, items):
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:     # the oracle's C calls drop the GIL
        return list(ex.map(fn, items))


def _zero_partner(S3, SA, x3, xa, rng):
    """a residue (y3, ya) whose pair with (x3, xa) scores exactly 0"""
    c = np.argwhere(S3[x3, :20][:, None] + SA[xa, :20][None, :] == 0)
    y3, ya = c[rng.integers(0, len(c))]
    return np.uint8(y3), np.uint8(ya)


def _mutate(rng, a3, aa, rate, indels=True):
    b3, ba = a3.copy(), aa.copy()
    m = rng.random(len(b3)) < rate
    b3[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
    m = rng.random(len(ba)) < rate
    ba[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
    if indels and len(b3) > 40:
        c = int(rng.integers(10, len(b3) // 2))
        b3, ba = np.delete(b3, slice(c, c + 3)), np.delete(ba, slice(c, c + 3))
        c = int(rng.integers(len(b3) // 2, len(b3) - 10))
        ins3, insa = rng.integers(0, 20, 4, dtype=np.uint8), rng.integers(0, 20, 4, dtype=np.uint8)
        b3, ba = np.concatenate([b3[:c], ins3, b3[c:]]), np.concatenate([ba[:c], insa, ba[c:]])
    return b3, ba


def _zigzag(rng, L):
    """q = A X B, t = A Y B with unrelated X, Y: the traceback leaves the corridor between its start and end diagonals (a gap out and back)"""
    def rnd(n): return rng.integers(0, 20, n, dtype=np.uint8), rng.integers(0, 20, n, dtype=np.uint8)
    lx, ly = int(rng.integers(8, 40)), int(rng.integers(8, 40))
    l1 = int(rng.integers(40, L - lx - 40))
    a, x, b, y = rnd(l1), rnd(lx), rnd(L - l1 - lx), rnd(ly)
    return (np.concatenate([a[0], x[0], b[0]]), np.concatenate([a[1], x[1], b[1]])), \
           (np.concatenate([a[0], y[0], b[0]]), np.concatenate([a[1], y[1], b[1]]))


def _sweep_lengths():
    Ls = set()
    for tab, caps in CAPS.items():
        lo = 1
        for cap in caps:
            Ls |= {lo, (lo + cap) // 2, cap}
            lo = cap + 1
    return sorted(Ls | {2049, 4300})           # the long-query kernel: one row block and a bit, more than two blocks


@pytest.fixture(scope="module")
def sweep(O):
    import unicore_amd as U
    p = O.default_params()
    dp = Dp(p)
    rng = np.random.default_rng(2024)
    s3, sa = [], []

    def add(x3, xa):
        s3.append(np.ascontiguousarray(x3, np.uint8)); sa.append(np.ascontiguousarray(xa, np.uint8))
        return len(s3) - 1

    unrel = {L: add(rng.integers(0, 20, L, dtype=np.uint8), rng.integers(0, 20, L, dtype=np.uint8)) for L in (1, 2, 63, 64, 65, 2100)}
    # queries with more pairs than one task holds: for every table and pairs-per-task value, the largest query of its first class
    split_extra = {}
    for tab in CAPS:
        for v in sorted(set(TCAP[tab])):
            L = CAPS[tab][TCAP[tab].index(v)]
            split_extra[L] = max(split_extra.get(L, 0), v + 1)
    split_extra[2049] = LONG_TASK + 3
    pairs, kinds = [], []
    for k, L in enumerate(_sweep_lengths()):
        q3, qa = rng.integers(0, 20, L, dtype=np.uint8), rng.integers(0, 20, L, dtype=np.uint8)
        q = add(q3, qa)
        tl = []
        tl.append((add(*_mutate(rng, q3, qa, 0.15)), "mutated"))
        pre = int(rng.integers(5, 30))
        sh3, sha = _mutate(rng, q3[L // 5:], qa[L // 5:], 0.1, indels=False)
        tl.append((add(np.concatenate([rng.integers(0, 20, pre, dtype=np.uint8), sh3]), np.concatenate([rng.integers(0, 20, pre, dtype=np.uint8), sha])), "shifted"))
        a = int(rng.integers(0, max(1, L - 40)))
        tl.append((add(*_mutate(rng, q3[a:a + 40], qa[a:a + 40], 0.05, indels=False)), "truncated"))
        if L >= 3:
            # last residue pair scores 0: two optimal rows in the forward DP (rows L-2 and L-1) - the ambiguous end row
            y3, ya = _zero_partner(dp.S3, dp.SA, q3[-1], qa[-1], rng)
            tl.append((add(np.append(q3[:-1], y3), np.append(qa[:-1], ya)), "zero-end"))
            # first residue pair scores 0: two optimal rows in the start pass's DP
            y3, ya = _zero_partner(dp.S3, dp.SA, q3[0], qa[0], rng)
            tl.append((add(np.insert(q3[1:], 0, y3), np.insert(qa[1:], 0, ya)), "zero-start"))
        else:
            tl.append((add(q3, qa), "self"))
            tl.append((add(*_mutate(rng, q3, qa, 0.3, indels=False)), "mutated"))
        tl.append((add(rng.integers(0, 20, L, dtype=np.uint8), rng.integers(0, 20, L, dtype=np.uint8)), "unrelated"))
        tl += [(unrel[x], "unrelated") for x in (63, 64, 65, 2100)]
        if k % 2 == 0:
            tl.append((unrel[1 if k % 4 == 0 else 2], "unrelated"))
        else:       # no 1- or 2-residue target: the task's shortest target - its lone last slot - is a related one
            a = int(rng.integers(0, max(1, L - 20)))
            tl.append((add(*_mutate(rng, q3[a:a + 20], qa[a:a + 20], 0.05, indels=False)), "truncated"))
        for _ in range(split_extra.get(L, 0) - len(tl) + (1 if (split_extra.get(L, 0) - len(tl)) % 2 else 0)):
            a, w = int(rng.integers(0, max(1, L - 60))), int(rng.integers(30, 61))
            tl.append((add(*_mutate(rng, q3[a:a + w], qa[a:a + w], 0.1, indels=False)), "fragment"))
        assert len(tl) % 2 == 1
        pairs += [(q, t) for t, _ in tl]
        kinds += [kd for _, kd in tl]
    # zig-zag pairs in classes of every group size of table 1 (G = 16, 32, 64)
    for L in (300, 500, 700, 1000, 1500):
        for _ in range(3):
            (a3, aa), (b3, ba) = _zigzag(rng, L)
            pairs.append((add(a3, aa), add(b3, ba)))
            kinds.append("zigzag")
    off, c3, ca = util.flat(s3, sa)
    e = U.Engine("-c 0.8", verbosity=1)
    e.set_db(off, c3, ca)
    odb = O.OracleDb(s3=s3, sa=sa)
    q = np.array([x[0] for x in pairs], np.uint32)
    t = np.array([x[1] for x in pairs], np.uint32)
    n = len(q)
    # oracle references, computed once: forward (modes 0 / 4), reversed query (1), reversed prefixes (2 / 6), traceback of the box (3 / 7)
    fwd = np.array(_pmap(lambda i: O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p), range(n)), np.int64).reshape(n, 3)
    rev = np.array(_pmap(lambda i: O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p, rev_q=1)[0], range(n)), np.int64)
    pos = np.nonzero(fwd[:, 0] > 0)[0]

    def start(i):
        qe, te = fwd[i, 1], fwd[i, 2]
        return O.sw(s3[q[i]][: qe + 1], sa[q[i]][: qe + 1], s3[t[i]][: te + 1], sa[t[i]][: te + 1], p, rev_q=1, rev_t=1)
    st = np.array(_pmap(start, pos), np.int64).reshape(len(pos), 3)
    assert np.array_equal(st[:, 0], fwd[pos, 0])          # the start pass reaches the forward optimum
    box = np.stack([fwd[pos, 1] - st[:, 1], fwd[pos, 1], fwd[pos, 2] - st[:, 2], fwd[pos, 2]], 1).astype(np.int32)
    tb = np.array(_pmap(lambda k: O.traceback(odb, p, q[pos[k]], t[pos[k]], *box[k]), range(len(pos))), np.int64).reshape(len(pos), 3)
    # numpy DP on the small pairs: rows holding an optimal cell, forward and start pass
    lens = np.array([len(x) for x in s3])
    small = [i for i in pos if lens[q[i]] <= 400 and lens[t[i]] <= 400]

    def rows(i):
        a, b = dp.summary(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]])
        qe, te = fwd[i, 1], fwd[i, 2]
        c, d = dp.summary(s3[q[i]][qe::-1], sa[q[i]][qe::-1], s3[t[i]][te::-1], sa[t[i]][te::-1])
        return a, len(b), c, len(d)
    dps = dict(zip(small, _pmap(rows, small)))
    for i, (a, nf, c, ns) in dps.items():                 # the numpy DP is the oracle's DP
        assert a == tuple(fwd[i]) and c == tuple(st[np.searchsorted(pos, i)]), i
    stats = {}
    return dict(e=e, p=p, dp=dp, s3=s3, sa=sa, odb=odb, q=q, t=t, n=n, kinds=np.array(kinds), lens=lens, fwd=fwd, rev=rev, pos=pos, st=st,
                box=box, tb=tb, dps=dps, stats=stats)


def _record(S, tab, mode, cls, sel, scores, flagged=None):
    """class histogram (pairs, pairs with score > 0, flagged pairs, pairs in a lone last slot) per (table, class, mode)"""
    q, lens = S["q"][sel], S["lens"]
    eff = _effective_target_lengths(S, mode, sel)
    lone = _lone_slots(tab, cls, q, eff)
    for c in np.unique(cls):
        m = cls == c
        h = S["stats"].setdefault((tab, int(c), mode), [0, 0, 0, 0])
        h[0] += int(m.sum()); h[1] += int((scores[m] > 0).sum())
        h[2] += int(flagged[m].sum()) if flagged is not None else 0
        h[3] += int(lone[m].sum())
    assert np.array_equal(cls, [class_of(int(lens[x]), tab) for x in q]), (tab, mode)


def _effective_target_lengths(S, mode, sel):
    if mode in (2, 6):
        return S["fwd"][sel, 2] + 1
    if mode in (3, 7):
        k = np.searchsorted(S["pos"], sel)
        return S["box"][k, 3] - S["box"][k, 2] + 1
    return S["lens"][S["t"][sel]]


def _lone_slots(tab, cls, q, eff):
    """pairs that run in a slot of their own (the last slot of a task with an odd pair count), as the planner cuts the list: per (class,
    query) segment, stable order by effective target length descending, tasks of TCAP pairs"""
    lone = np.zeros(len(q), bool)
    keys = {}
    for i in range(len(q)):
        keys.setdefault((int(cls[i]), int(q[i])), []).append(i)
    for (c, _), idx in keys.items():
        if c >= len(CAPS[tab]):
            continue
        order = sorted(idx, key=lambda i: -int(eff[i]))
        cap = TCAP[tab][c]
        for b in range(0, len(order), cap):
            chunk = order[b:b + cap]
            if len(chunk) % 2:
                lone[chunk[-1]] = True
    return lone


@pytest.fixture(scope="module")
def runs(sweep):
    """every pass of the sweep, once: R[(table, mode[, band])] (raw runs: mode "0raw" / "7raw"); the class histogram in S["stats"]"""
    S = sweep
    e, q, t, fwd, pos = S["e"], S["q"], S["t"], S["fwd"], S["pos"]
    allp = np.arange(S["n"])
    known = fwd[pos, 0].astype(np.int32)
    ends = np.zeros((len(pos), 4), np.int32)
    ends[:, 1], ends[:, 3] = fwd[pos, 1], fwd[pos, 2]
    R = {}
    for tab in (0, 1):
        R[tab, 0] = e.sw_pass(tab, 0, q, t)
        _record(S, tab, 0, R[tab, 0]["cls"], allp, R[tab, 0]["score"])
        R[tab, 1] = e.sw_pass(tab, 1, q, t)
        _record(S, tab, 1, R[tab, 1]["cls"], allp, R[tab, 1]["score"])
        R[tab, 2] = e.sw_pass(tab, 2, q[pos], t[pos], box=ends)
        _record(S, tab, 2, R[tab, 2]["cls"], pos, R[tab, 2]["score"])
    r = R[1, "0raw"] = e.sw_pass(1, 0, q, t, raw=True)
    _record(S, 1, "0raw", r["cls"], allp, r["score"], (r["qe"] == -2) | (r["score"] >= SW_PK_OVF))
    for tab in (1, 3):      # known-score passes, raw: the packed kernel's own answers (no pair here reaches the packed range limit)
        R[tab, 4] = e.sw_pass(tab, 4, q[pos], t[pos], known=known, raw=True)
        _record(S, tab, 4, R[tab, 4]["cls"], pos, R[tab, 4]["score"])
        r = R[tab, 6] = e.sw_pass(tab, 6, q[pos], t[pos], box=ends, known=known, raw=True)
        _record(S, tab, 6, r["cls"], pos, r["score"], (r["te"] >= 0) & ((r["te"] & TE_UNIQUE) == 0))
    for W in BANDS:
        r = R[1, 7, W] = e.sw_pass(1, 7, q[pos], t[pos], box=S["box"], known=known, band=W)
        _record(S, 1, 7, r["cls"], pos, r["score"], r["miss"] != 0)
    R[1, "7raw", 1] = e.sw_pass(1, 7, q[pos], t[pos], box=S["box"], known=known, band=1, raw=True)
    R[2, 3] = e.sw_pass(2, 3, q[pos], t[pos], box=S["box"])
    _record(S, 2, 3, R[2, 3]["cls"], pos, S["tb"][:, 0])
    return R


def test_class_sweep_forward_reverse_start(sweep, runs):
    """tables 0 (int32) and 1 (packed, with the library's re-run rules) in modes 0, 1, 2: every class, both edges, the long-query kernel"""
    S = sweep
    for tab in (0, 1):
        r = runs[tab, 0]
        assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1), S["fwd"]), tab
        assert np.array_equal(runs[tab, 1]["score"], S["rev"]), tab
        r = runs[tab, 2]
        assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1), S["st"]), tab
    L = S["lens"][S["q"]]
    assert (L > 4096).any() and (L == 2049).any()


def test_raw_packed_forward_flags(sweep, runs):
    """raw MODE 0 of the packed kernel: every pair it does not flag has the oracle's score and ends; every pair flagged with an
    ambiguous end row (qe = -2) really has more than one optimal row, and every small pair with several optimal rows is flagged"""
    S = sweep
    fwd, dps, kinds = S["fwd"], S["dps"], S["kinds"]
    r = runs[1, "0raw"]
    flagged = (r["qe"] == -2) | (r["score"] >= SW_PK_OVF)
    ok = ~flagged
    assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1)[ok], fwd[ok])
    assert np.array_equal(r["score"], fwd[:, 0])          # the scores are exact even where the end row is not
    amb = np.nonzero(r["qe"] == -2)[0]
    s3, sa, q, t = S["s3"], S["sa"], S["q"], S["t"]
    big = [i for i in amb if i not in dps]                # the larger flagged pairs: their numpy DP here

    def nrows(i):
        return len(S["dp"].summary(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]])[1])
    for i, nr in zip(big, _pmap(nrows, big)):
        assert nr > 1, i
    checked = 0
    for i in amb:
        if i in dps:
            assert dps[i][1] > 1, i
            checked += 1
    for i, (a, nf, c, ns) in dps.items():
        assert (r["qe"][i] == -2) == (nf > 1), i
    assert checked >= 20 and (kinds[amb] == "zero-end").sum() >= 40, (checked, (kinds[amb] == "zero-end").sum())


@pytest.mark.parametrize("tab", [1, 3])
def test_known_score_passes(sweep, runs, tab):
    """MODE 4 (forward, optimum known) and MODE 6 (start pass, optimum known) of the packed kernel, raw: the oracle's ends on every pair; the
    one-row mark of MODE 6 exactly when one row of the start pass's DP holds every optimal cell (numpy DP).  Table 3 (the sparse plans)
    forced, whatever the pairs per query"""
    S = sweep
    q, fwd, pos, st, dps = S["q"], S["fwd"], S["pos"], S["st"], S["dps"]
    r = runs[tab, 4]
    assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1), fwd[pos]), tab
    amb4 = sum(1 for i in pos if i in dps and dps[i][1] > 1)
    r = runs[tab, 6]
    uniq = (r["te"] >= 0) & ((r["te"] & TE_UNIQUE) != 0)
    te = np.where(r["te"] >= 0, r["te"] & ~TE_UNIQUE, r["te"])
    assert np.array_equal(np.stack([r["score"], r["qe"], te], 1), st), tab
    both = {True: 0, False: 0}
    long_q = S["lens"][q[pos]] > 2048
    for k, i in enumerate(pos):
        if i in dps and not long_q[k]:
            single = dps[i][3] == 1
            assert uniq[k] == single, (tab, i, S["kinds"][i], dps[i])
            both[single] += 1
    assert not uniq[long_q].any()                       # the int32 long-query kernel never sets it
    assert both[True] >= 50 and both[False] >= 20 and amb4 >= 20, (both, amb4)


def test_traceback_bytes_and_int32_statistics(sweep, runs):
    """MODE 7 (H bytes of a diagonal band + walk) on every class of table 1 for W = 0, 1, 4, 48, and table 2 in MODE 3 (both weightings):
    (alignment length, identities, gap opens) of the oracle's traceback on the oracle's box.  W = 1: some walks leave the band, and after
    the library's fallback (the whole box) they are exact; raw, they report the miss and leave the statistics alone"""
    S = sweep
    q, pos, tb, dps = S["q"], S["pos"], S["tb"], S["dps"]
    for W in BANDS:
        r = runs[1, 7, W]
        got = np.stack([r["aln_len"], r["idents"], r["gaps"]], 1)
        assert np.array_equal(got, tb), (W, np.nonzero((got != tb).any(1))[0][:10])
        if W == 0:
            assert not r["miss"].any()
    miss = runs[1, 7, 1]["miss"] != 0
    zz = S["kinds"][pos] == "zigzag"
    g = S["lens"][q[pos]]
    assert miss.sum() >= 10 and miss[zz].sum() >= 5, (miss.sum(), miss[zz].sum())
    assert (miss & zz & (g > 384) & (g <= 768)).any() and (miss & zz & (g > 768) & (g <= 2048)).any()      # G = 32 and G = 64 classes
    raw = runs[1, "7raw", 1]
    rm = raw["miss"] != 0
    assert np.array_equal(rm, miss)
    assert (raw["aln_len"][rm] == -1).all()
    assert np.array_equal(np.stack([raw["aln_len"], raw["idents"], raw["gaps"]], 1)[~rm], tb[~rm])
    # boxes of pairs whose forward end row is ambiguous went through the walk too
    assert sum(1 for i in pos if i in dps and dps[i][1] > 1) >= 20
    r = runs[2, 3]
    assert np.array_equal(np.stack([r["aln_len"], r["idents"], r["gaps"]], 1), tb)
    assert (tb[:, 2] > 0).sum() >= 50                     # gapped tracebacks, not only diagonals


def test_every_class_and_mode_ran(sweep, runs):
    """not vacuous: every (table, class, allowed mode) ran on a pair with score > 0 and in a lone last slot; the histogram goes to the log"""
    S = sweep
    for tab, modes in MODES.items():
        for mode in modes:
            for c in range(len(CAPS[tab]) + 1):
                h = S["stats"].get((tab, c, mode))
                assert h is not None and h[1] > 0, (tab, c, mode)
                if c < len(CAPS[tab]):
                    assert h[3] > 0, ("no lone slot", tab, c, mode)
    assert sum(h[2] for k, h in S["stats"].items() if k[2] == "0raw") >= 40
    assert sum(h[2] for k, h in S["stats"].items() if k[2] == 6) >= 20        # MODE 6 pairs without the one-row mark
    print("\nclass histogram - (table, class, mode): [pairs, score > 0, flagged, lone slot]")
    for k in sorted(S["stats"], key=str):
        print("  %s: %s" % (k, S["stats"][k]))


def test_sw_pass_rejects_invalid_input(sweep):
    import unicore_amd as U
    S = sweep
    e, q, t = S["e"], S["q"][:3], S["t"][:3]
    L = S["lens"]
    known = np.ones(3, np.int32)
    okbox = np.zeros((3, 4), np.int32)
    bad = [dict(table=0, mode=4, known=known), dict(table=2, mode=0), dict(table=3, mode=0), dict(table=1, mode=3, box=okbox),
           dict(table=4, mode=0), dict(table=1, mode=5), dict(table=1, mode=4), dict(table=1, mode=6, box=okbox),
           dict(table=1, mode=7, box=okbox), dict(table=1, mode=2),
           dict(table=1, mode=4, known=np.zeros(3, np.int32)),
           dict(table=1, mode=2, box=np.array([[0, L[x], 0, 0] for x in q], np.int32)),
           dict(table=2, mode=3, box=np.array([[1, 0, 0, 0]] * 3, np.int32)),
           dict(table=2, mode=3, box=np.array([[0, 0, 0, L[x]] for x in t], np.int32)),
           dict(table=1, mode=7, box=okbox, known=known, band=-1)]
    for kw in bad:
        tab, mode = kw.pop("table"), kw.pop("mode")
        with pytest.raises(U.UcError) as ei:
            e.sw_pass(tab, mode, q, t, **kw)
        assert ei.value.code == U.UC_ERR_ARGS, (tab, mode, kw)
    with pytest.raises(U.UcError) as ei:
        e.sw_pass(0, 0, np.array([len(S["s3"]) + 5], np.uint32), t[:1])
    assert ei.value.code == U.UC_ERR_ARGS


def _scaled_matrix(src, dst, factor):
    out = []
    for line in open(src):
        tok = line.split()
        if line.startswith("#") or not tok or not tok[0].isalpha() or len(tok) < 3 or not tok[1].lstrip("-").isdigit():
            out.append(line)
        else:
            out.append(tok[0] + " " + " ".join(str(max(-48, min(48, int(v) * factor))) for v in tok[1:]) + "\n")
    open(dst, "w").writelines(out)


def test_packed_range_edge(O, tmp_path):
    """scores on both sides of the packed range limits: SW_PK_OVF - 1, SW_PK_OVF (re-run from here on), 0x7C00 - 1, 0x7C00 (the f16
    infinity pattern) and far beyond, on self and near-self pairs (3Di matrix scaled 4x; the AA matrix as is, so every integer is
    reachable).  Modes 0, 1 (reversed copies), 2 and 7 (the top ones go to int32 MODE 3) are exact; raw MODE 0 is exact below
    SW_PK_OVF and flags everything at or above it"""
    import unicore_amd as U
    m3 = str(tmp_path / "m3.out")
    _scaled_matrix(os.path.join(util.ROOT, "unicore_amd", "data", "mat3di_synthetic.out"), m3, 4)
    p = O.default_params()
    assert O.lib().uco_load_matrix(m3.encode(), p.S3) == 0
    S3 = np.array(p.S3[:], np.int32).reshape(21, 21)
    SA = np.array(p.SA[:], np.int32).reshape(21, 21)
    rng = np.random.default_rng(5)
    targets = [SW_PK_OVF - 1, SW_PK_OVF, 0x7C00 - 1, 0x7C00, 0x7C00 + 4321, 45000]
    s3, sa, pairs, want = [], [], [], []
    for k, T in enumerate(targets):
        for letters in (np.arange(20), np.argsort(-np.diag(S3)[:20])[:6]):       # all letters, and the six highest 3Di self-scores
            b3 = rng.choice(letters, 2100).astype(np.uint8)
            ba = rng.integers(0, 20, 2100, dtype=np.uint8)
            d = S3[b3, b3] + SA[ba, ba]
            L = int(np.searchsorted(np.cumsum(d), T)) + 1
            if L > 2048:
                continue
            b3, ba = b3[:L], ba[:L]
            delta = int(d[:L].sum()) - T
            c3, ca = b3.copy(), ba.copy()
            if delta:   # one substitution in the middle half takes exactly delta off the diagonal
                for i in range(L // 2, 3 * L // 4):
                    cand = np.argwhere(d[i] - (S3[b3[i], :20][:, None] + SA[ba[i], :20][None, :]) == delta)
                    if len(cand):
                        c3[i], ca[i] = cand[0]
                        break
                else:
                    raise AssertionError((T, delta))
            qi = len(s3); s3 += [b3, c3, c3[::-1].copy()]; sa += [ba, ca, ca[::-1].copy()]
            pairs.append((qi, qi + 1, qi + 2)); want.append(T)
            if not delta:
                pairs.append((qi, qi, qi + 2)); want.append(T)
    off, c3_, ca_ = util.flat(s3, sa)
    e = U.Engine("-c 0.8 --mat3di %s" % m3, verbosity=1)
    e.set_db(off, c3_, ca_)
    q = np.array([x[0] for x in pairs], np.uint32); t = np.array([x[1] for x in pairs], np.uint32); tr = np.array([x[2] for x in pairs], np.uint32)
    fwd = np.array([O.sw(s3[a], sa[a], s3[b], sa[b], p) for a, b in zip(q, t)])
    assert np.array_equal(fwd[:, 0], want)                    # the construction lands on the edges
    assert len(set(want)) == len(targets)
    rev = np.array([O.sw(s3[a], sa[a], s3[b], sa[b], p, rev_q=1)[0] for a, b in zip(q, tr)])
    assert np.array_equal(rev, want)
    st = np.array([O.sw(s3[a][: x[1] + 1], sa[a][: x[1] + 1], s3[b][: x[2] + 1], sa[b][: x[2] + 1], p, rev_q=1, rev_t=1) for a, b, x in zip(q, t, fwd)])
    r = e.sw_pass(1, 0, q, t)
    assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1), fwd)
    raw = e.sw_pass(1, 0, q, t, raw=True)
    lo = fwd[:, 0] < SW_PK_OVF
    assert np.array_equal(np.stack([raw["score"], raw["qe"], raw["te"]], 1)[lo], fwd[lo])
    assert (raw["score"][~lo] >= SW_PK_OVF).all() and lo.any() and (~lo).any()
    assert np.array_equal(e.sw_pass(1, 1, q, tr)["score"], rev)
    assert (e.sw_pass(1, 1, q, tr, raw=True)["score"][~lo] >= SW_PK_OVF).all()
    bx = np.zeros((len(q), 4), np.int32)
    bx[:, 1], bx[:, 3] = fwd[:, 1], fwd[:, 2]
    r = e.sw_pass(1, 2, q, t, box=bx)
    assert np.array_equal(np.stack([r["score"], r["qe"], r["te"]], 1), st)
    odb = O.OracleDb(s3=s3, sa=sa)
    box = np.stack([fwd[:, 1] - st[:, 1], fwd[:, 1], fwd[:, 2] - st[:, 2], fwd[:, 2]], 1).astype(np.int32)
    tb = np.array([O.traceback(odb, p, a, b, *x) for a, b, x in zip(q, t, box)])
    for W in (0, 48):
        r = e.sw_pass(1, 7, q, t, box=box, known=fwd[:, 0].astype(np.int32), band=W)
        assert np.array_equal(np.stack([r["aln_len"], r["idents"], r["gaps"]], 1), tb), W
