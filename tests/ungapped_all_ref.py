"""Rule UC-1/X (--prefilter-mode 1) restated in numpy, for tests/test_prefilter_mode1*.py.

E3x of one query against a list of targets: for every diagonal d in -(Lt-1) .. Lq-1 the E3 score u(d) (Kadane along the diagonal on
S3[q3[i]][t3[i-d]] (+ the query position's compositional bias), best of the run, capped at 255); the pair's score is max_d u(d), its diagonal the
smallest d that reaches that maximum.  A pair with an EMPTY sequence has no cell and no diagonal: score 0, diag 0, and it is in no hit list whatever
the threshold.  One vector update per query row over an (n_targets x Lmax) array."""
import ctypes as C

import numpy as np


def matrix(p):
    return np.array(list(p.S3), dtype=np.int32).reshape(21, 21)


def comp_bias(O, q3, p):
    """rule UC-1/B through the oracle (uco_comp_bias); zeros when the rule is off"""
    q3 = np.ascontiguousarray(q3, np.uint8)
    out = np.zeros(len(q3), np.int8)
    if p.comp_bias_milli and len(q3):
        f = O.lib().uco_comp_bias
        f.restype = None
        f(C.c_void_p(q3.ctypes.data), C.c_int(len(q3)), p.S3, C.c_int(p.comp_bias_milli), C.c_void_p(out.ctypes.data))
    return out.astype(np.int32)


def oracle_ungapped_bias(O, q3, t3, diag, p, bias):
    q3 = np.ascontiguousarray(q3, np.uint8); t3 = np.ascontiguousarray(t3, np.uint8)
    b = np.ascontiguousarray(bias, np.int8)
    f = O.lib().uco_ungapped_bias
    f.restype = C.c_int32
    return int(f(C.c_void_p(q3.ctypes.data), C.c_int(len(q3)), C.c_void_p(t3.ctypes.data), C.c_int(len(t3)), C.c_int(int(diag)), p.S3,
                 C.c_void_p(b.ctypes.data) if p.comp_bias_milli else None))


def _group(q3, bias, tg, S):
    """targets of similar length as one padded array -> best[nt, Lq + Lmax - 1] (index d + Lmax - 1), uncapped"""
    nt, lq = len(tg), len(q3)
    lens = np.array([len(t) for t in tg])
    lmax = int(lens.max())
    T = np.full((nt, lmax), 20, np.int64)
    for k, t in enumerate(tg):
        T[k, :len(t)] = t
    inside = np.arange(lmax)[None, :] < lens[:, None]
    run = np.zeros((nt, lmax), np.int32)
    best = np.zeros((nt, lq + lmax - 1), np.int32)
    for i in range(lq):
        sc = S[int(q3[i])][T] + int(bias[i])
        prev = np.zeros_like(run)
        prev[:, 1:] = run[:, :-1]                      # cell (i - 1, j - 1): the same diagonal
        run = np.where(inside, np.maximum(prev + sc, 0), 0).astype(np.int32)
        view = best[:, i:i + lmax][:, ::-1]            # column j of the row lies on diagonal i - j: index i - j + lmax - 1
        np.maximum(view, run, out=view)
    return best, lens, lmax


def e3x(q3, bias, targets, S, long_len=512):
    """(score[nt], diag[nt]) of one query against `targets` (list of code arrays)"""
    nt, lq = len(targets), len(q3)
    score, diag = np.zeros(nt, np.int32), np.zeros(nt, np.int32)
    if lq == 0:
        return score, diag
    short = [k for k in range(nt) if 0 < len(targets[k]) <= long_len]            # (empty targets keep score 0, diag 0)
    groups = ([short] if short else []) + [[k] for k in range(nt) if len(targets[k]) > long_len]
    for g in groups:
        best, lens, lmax = _group(q3, bias, [targets[k] for k in g], S)
        d = np.arange(lq + lmax - 1)[None, :] - (lmax - 1)
        u = np.where(d >= -(lens[:, None] - 1), np.minimum(best, 255), -1)       # diagonals the pair does not have never win
        a = np.argmax(u, axis=1)                       # first maximum = smallest diagonal
        score[g] = u[np.arange(len(g)), a]
        diag[g] = a - (lmax - 1)
    return score, diag


def dense(O, s3, p, queries, targets):
    """[len(queries), len(targets)] score and diag arrays for sequence ids of the database s3"""
    S = matrix(p)
    sc = np.zeros((len(queries), len(targets)), np.int32)
    dg = np.zeros_like(sc)
    tg = [s3[t] for t in targets]
    for k, q in enumerate(queries):
        sc[k], dg[k] = e3x(s3[q], comp_bias(O, s3[q], p), tg, S)
    return sc, dg


def hit_lists(score, diag, targets, min_ungapped, max_seqs, lens=None, queries=None):
    """threshold + order (score desc, target asc) + truncate: per query a list of (target, score, diag).  lens (sequence lengths by id; queries = the ids of
    the rows, default = targets' numbering from 0): empty sequences are in no list"""
    out = []
    for k in range(score.shape[0]):
        if lens is not None and lens[queries[k] if queries is not None else k] == 0:
            out.append([])
            continue
        keep = [(int(targets[j]), int(score[k, j]), int(diag[k, j])) for j in range(score.shape[1])
                if score[k, j] >= min_ungapped and (lens is None or lens[targets[j]] > 0)]
        keep.sort(key=lambda h: (-h[1], h[0]))
        out.append(keep[:max_seqs])
    return out


def mode1_db(seed=11):
    """~128 sequences: length 0, length 1, below the k-mer span, 50-400, one of ~5,000 (id 0), X residues, an identical pair, a periodic pair that reaches 255 on
    several diagonals, a 6-residue substring of another sequence.  Returns (s3, sa, info)."""
    rng = np.random.default_rng(seed)
    rnd = lambda L: rng.integers(0, 20, L, dtype=np.uint8)
    s3, sa = [rnd(5003)], [rnd(5003)]                                       # 0: the long one (a query and a target)
    motif = rnd(7)
    s3 += [np.tile(motif, 40), np.tile(motif, 43)]; sa += [rnd(280), rnd(301)]   # 1, 2: periodic - many diagonals beyond the cap
    base3, basea = rnd(180), rnd(180)
    s3 += [base3, base3.copy()]; sa += [basea, basea.copy()]                # 3, 4: identical
    s3 += [base3[40:46].copy()]; sa += [basea[40:46].copy()]                        # 5: length 6, a substring of 3 and 4
    for L in (1, 1, 5, 9, 2):                                               # 6..10: length 1 and below the span
        s3.append(rnd(L)); sa.append(rnd(L))
    x3 = rnd(120); x3[10:30] = 20
    s3.append(x3); sa.append(rnd(120))                                      # 11: a run of X
    s3.append(np.full(15, 20, np.uint8)); sa.append(np.full(15, 20, np.uint8))   # 12: all X
    s3.append(np.zeros(0, np.uint8)); sa.append(np.zeros(0, np.uint8))          # 13: EMPTY (the engine accepts zero-length entries)
    while len(s3) < 128:                                                    # families of mutated members, 50-400
        L = int(rng.integers(50, 401))
        a3, aa = rnd(L), rnd(L)
        for m in range(6):
            if len(s3) >= 128:
                break
            keep = rng.random(L) >= 0.02
            m3, ma = a3[keep].copy(), aa[keep].copy()
            mu3, mua = rng.random(len(m3)) < 0.15, rng.random(len(ma)) < 0.3
            m3[mu3] = rng.integers(0, 20, int(mu3.sum()), dtype=np.uint8)
            ma[mua] = rng.integers(0, 20, int(mua.sum()), dtype=np.uint8)
            if m == 2:
                m3[7] = 20; ma[3] = 20
            if m == 5:
                m3, ma = m3[:int(len(m3) * 0.6)], ma[:int(len(ma) * 0.6)]
            s3.append(m3); sa.append(ma)
    return s3, sa, dict(long=0, periodic=(1, 2), identical=(3, 4), short=5, empty=13)
