"""Cases and checks of tests/test_sw_bias_gpu.py: the packed gapped kernels in the biased score domain (H' = H + 128, E' = E + 128 in every mode
but 7), one pass at a time through Engine.sw_pass against the scalar oracle - exact integers.  The shapes are the smallest that can break it:

  query lengths 1, 2, R, R + 1, G R - 1, G R of one class per lane-group width (table 1: (16, 2), (16, 12), (32, 14), (64, 14); table 3: (64, 2));
  target lengths 1, 2, 63, 64, 65, and related targets (a mutated window of the query at its start and at its end: < 150 residues, so that a score stays
      in the packed range); substitution matrices scaled to the option limit of +-48 per track (-96 .. +96 per cell);
  pairs without a positive cell (score 0, ends -1); the optimum in the first row, and in the first column; an optimum of exactly 1, in one cell and
      in every row of a column; start-pass boxes whose first unmasked row is the first row of a lane, the last row of the lane before, and one further;
  a slot of one pair above 0x7C00 and one ordinary pair, the overflowing one as the longer target (low half) and as the shorter one (high half).

Run as a program (argv: a scratch directory) it builds the same cases and runs every check for both gap settings in a process of its own:
UC_SW_TASK_QUERIES is read once per process.  Prints `multiquery_launches=N`."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")

import matrix_cases as MC      # noqa: E402
import util                    # noqa: E402

SW_PK_OVF = 0x7C00 - 256
TE_UNIQUE = 1 << 30
GAPS = ((31, 1), (1, 0))       # (open, extend): the widest gap-open the options take, and the narrowest with a free extension
QUERY_LENGTHS = (1, 2, 3, 12, 13, 14, 15, 31, 32, 127, 128, 191, 192, 447, 448, 895, 896)
CLASS_OF_BOX = ((32, 2), (192, 12), (448, 14), (896, 14))      # (query length, R of its class): where the start-pass boxes are cut


def scaled_matrices(O):
    """the shipped matrices scaled until both tracks reach +48 and -48, clipped there; one letter pair (u, v) scores exactly 1"""
    S3, SA = MC.base(O)
    out = []
    for M in (S3, SA):
        f = -(-48 // min(int(M[:20, :20].max()), -int(M[:20, :20].min())))
        M = np.clip(M * f, -48, 48)
        assert M[:20, :20].max() == 48 and M[:20, :20].min() == -48
        out.append(M)
    S3, SA = out
    tot = S3 + SA
    hot = [a for a in range(20) if tot[a, a] == 96]
    hot3, hota = [a for a in range(20) if S3[a, a] == 48], [a for a in range(20) if SA[a, a] == 48]
    assert hot and len(hot3) >= 2 and len(hota) >= 2, (hot, hot3, hota)
    # letters x, y, w, u, v: every pair among them negative but (u, v), which is set to 1
    neg = lambda a, b: tot[a, b] < 0 and tot[b, a] < 0
    for x in hot:
        rest = [a for a in range(20) if a != x and neg(a, x)]
        pick = [x]
        for a in rest:
            if all(neg(a, b) for b in pick):
                pick.append(a)
            if len(pick) == 5:
                break
        if len(pick) == 5:
            break
    else:
        raise AssertionError("no five mutually negative letters")
    x, y, w, u, v = pick
    S3[u, v] = S3[v, u] = 1
    SA[u, v] = SA[v, u] = 0
    z1, z2 = [a for a in range(20) if a not in pick][:2]           # and one pair at the lower limit on both tracks
    S3[z1, z2] = S3[z2, z1] = SA[z1, z2] = SA[z2, z1] = -48
    tot = (S3 + SA)[:20, :20]
    assert tot.max() == 96 and tot.min() == -96
    return S3, SA, dict(x=x, y=y, w=w, u=u, v=v, hot3=hot3, hota=hota)


def build(O, tmp_dir):
    S3, SA, L = scaled_matrices(O)
    mats = "--mat3di %s --mat-aa %s" % (MC.write_matrix(os.path.join(str(tmp_dir), "bias_3di.out"), S3), MC.write_matrix(os.path.join(str(tmp_dir), "bias_aa.out"), SA))
    rng = np.random.default_rng(4242)
    s3, sa, pairs, kinds, boxes = [], [], [], [], []

    def add(a3, aa=None):
        a3 = np.ascontiguousarray(a3, np.uint8)
        s3.append(a3); sa.append(a3.copy() if aa is None else np.ascontiguousarray(aa, np.uint8))
        return len(s3) - 1

    def rnd(n):
        return rng.integers(0, 20, n, dtype=np.uint8), rng.integers(0, 20, n, dtype=np.uint8)

    def mutated(a3, aa, rate=0.12):
        b3, ba = a3.copy(), aa.copy()
        m = rng.random(len(b3)) < rate
        b3[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
        m = rng.random(len(ba)) < rate
        ba[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
        if len(b3) > 30:
            c = int(rng.integers(8, len(b3) - 8))
            b3, ba = np.delete(b3, slice(c, c + 2)), np.delete(ba, slice(c, c + 2))
        return b3, ba

    def pair(q, t, kind):
        pairs.append((q, t)); kinds.append(kind)

    unrel = {n: add(*rnd(n)) for n in (1, 2, 63, 64, 65)}
    qid = {}
    for n in QUERY_LENGTHS:
        q3, qa = rnd(n)
        q = qid[n] = add(q3, qa)
        for m in (1, 2, 63, 64, 65):
            pair(q, unrel[m], "unrelated")
        wlen = min(n, 140)
        pair(q, add(*mutated(q3[:wlen], qa[:wlen])), "window-start")
        e3, ea = mutated(q3[n - wlen:], qa[n - wlen:])
        pre = rnd(int(rng.integers(3, 20)))
        pair(q, add(np.concatenate([pre[0], e3]), np.concatenate([pre[1], ea])), "window-end")
        if n % 2:
            pair(q, add(q3[:1], qa[:1]), "first-residue")       # a one-residue target equal to the query's first residue
    x, y, w, u, v = (np.uint8(L[k]) for k in "xywuv")
    rep = lambda a, n: np.full(n, a, np.uint8)
    for n in (13, 192):
        pair(add(rep(x, n)), add(rep(y, 20)), "no-positive-cell")
        pair(add(rep(y, n)), add(rep(w, 1)), "no-positive-cell")
        pair(add(np.concatenate([rep(x, 1), rep(y, n - 1)])), add(np.concatenate([rep(w, 5), rep(x, 1)])), "first-row")
        k = n // 2
        pair(add(np.concatenate([rep(y, k), rep(x, 1), rep(y, n - k - 1)])), add(np.concatenate([rep(x, 1), rep(w, 5)])), "first-column")
        pair(add(rep(u, n)), add(rep(v, 1)), "score-1-every-row")
        pair(add(np.concatenate([rep(y, k), rep(u, 1), rep(y, n - k - 1)])), add(np.concatenate([rep(w, 2), rep(v, 1), rep(w, 2)])), "score-1-one-cell")
    # the overflowing slots: a query of 350 residues over the letters whose self score is 48 on their track, its copy (33,600 > 0x7C00) and ONE ordinary partner
    for tag, plen in (("ovf-high-half", 400), ("ovf-low-half", 60)):
        o3, oa = rng.choice(L["hot3"], 350).astype(np.uint8), rng.choice(L["hota"], 350).astype(np.uint8)
        q = add(o3, oa)
        cp = add(o3, oa)
        pair(q, cp, tag)
        a = int(rng.integers(0, 250))
        f3, fa = mutated(o3[a:a + 60], oa[a:a + 60])
        fill = rnd(plen - len(f3))
        pt = add(np.concatenate([fill[0][: len(fill[0]) // 2], f3, fill[0][len(fill[0]) // 2:]]),
                 np.concatenate([fill[1][: len(fill[1]) // 2], fa, fill[1][len(fill[1]) // 2:]]))
        pair(q, pt, tag + "-partner")
        qr = add(o3[::-1], oa[::-1])            # the same slot for the reversed-query pass: the reversed query against the copy
        pair(qr, cp, tag + "-rev")
        pair(qr, pt, tag + "-rev-partner")
    # start-pass boxes cut by hand: the reversed-prefix DP of rows [0, qe]; its first unmasked row is rowoff = lq - 1 - qe
    for n, R in CLASS_OF_BOX:
        q = qid[n]
        t = add(*mutated(s3[q][n - min(n, 140):], sa[q][n - min(n, 140):]))
        for rowoff in (R, R - 1, R + 1, 2 * R, 1):
            if rowoff < n - 1:
                boxes.append((q, t, n - 1 - rowoff, len(s3[t]) - 1 - (rowoff % 3)))
    lens = np.array([len(a) for a in s3])
    return dict(s3=s3, sa=sa, mats=mats, lens=lens, kinds=np.array(kinds), q=np.array([a for a, _ in pairs], np.uint32), t=np.array([b for _, b in pairs], np.uint32),
                boxes=np.array(boxes, np.int64), letters=L)


def options(C, gap):
    return "-c 0.8 %s --gap-open %d --gap-extend %d" % (C["mats"], gap[0], gap[1])


def references(O, C, gap):
    """the oracle's answers: forward (score, qe, te), reversed-query score, the start pass on the forward ends and on the hand-cut boxes"""
    p = util.oracle_params(O, options(C, gap))
    assert (p.gap_open, p.gap_ext) == gap
    s3, sa, q, t = C["s3"], C["sa"], C["q"], C["t"]
    n = len(q)
    fwd = np.array([O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p) for i in range(n)], np.int64).reshape(n, 3)
    rev = np.array([O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p, rev_q=1)[0] for i in range(n)], np.int64)

    def start(a, b, qe, te):
        return O.sw(s3[a][: qe + 1], sa[a][: qe + 1], s3[b][: te + 1], sa[b][: te + 1], p, rev_q=1, rev_t=1)
    pos = np.nonzero(fwd[:, 0] > 0)[0]
    st = np.array([start(q[i], t[i], fwd[i, 1], fwd[i, 2]) for i in pos], np.int64).reshape(len(pos), 3)
    bst = np.array([start(*b) for b in C["boxes"]], np.int64).reshape(len(C["boxes"]), 3)
    return dict(p=p, fwd=fwd, rev=rev, pos=pos, st=st, bst=bst)


def cases_are_what_they_claim(C, Rf):
    fwd, kinds = Rf["fwd"], C["kinds"]
    k = lambda name: np.nonzero(kinds == name)[0]
    assert (fwd[k("no-positive-cell")] == [0, -1, -1]).all()
    assert (fwd[k("first-row"), 1] == 0).all() and (fwd[k("first-row"), 2] == 5).all() and (fwd[k("first-row"), 0] == 96).all()
    assert (fwd[k("first-column"), 2] == 0).all() and (fwd[k("first-column"), 1] > 0).all()
    assert (fwd[k("score-1-every-row")] == [1, 0, 0]).all() and (fwd[k("score-1-one-cell"), 0] == 1).all() and (fwd[k("score-1-one-cell"), 2] == 2).all()
    for tag in ("ovf-high-half", "ovf-low-half"):
        (i,), (j,) = k(tag), k(tag + "-partner")
        assert fwd[i, 0] >= 0x7C00 and 0 < fwd[j, 0] < SW_PK_OVF and C["q"][i] == C["q"][j]
        longer = C["lens"][C["t"][j]] > C["lens"][C["t"][i]]
        assert longer == (tag == "ovf-high-half")         # a slot's first pair (the low half) is the longer target
    # every other pair stays inside the packed range
    assert (fwd[~np.isin(kinds, ("ovf-high-half", "ovf-low-half")), 0] < SW_PK_OVF).all()
    rv = np.isin(kinds, ("ovf-high-half-rev", "ovf-low-half-rev"))
    assert (Rf["rev"][rv] >= 0x7C00).all() and rv.sum() == 2 and (Rf["rev"][~rv] < SW_PK_OVF).all()
    assert (Rf["bst"][:, 0] > 0).sum() >= len(Rf["bst"]) - 2
    assert (fwd[kinds == "window-end", 0] > 0).all()


def engine(U, C, gap):
    e = U.Engine(options(C, gap), verbosity=1)
    e.set_db(*util.flat(C["s3"], C["sa"]))
    return e


def _triple(r, mask_unique=False):
    te = np.where(r["te"] >= 0, r["te"] & ~TE_UNIQUE, r["te"]) if mask_unique else r["te"]
    return np.stack([r["score"], r["qe"], te], 1)


def _same(got, want, what):
    bad = np.nonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(1))[0]
    assert not len(bad), (what, bad[:8].tolist(), np.asarray(got)[bad[:4]].tolist(), np.asarray(want)[bad[:4]].tolist())


def check_forward(e, C, Rf):
    """MODE 0 with the library's re-run rules, and raw: the kernel's own answers"""
    q, t, fwd = C["q"], C["t"], Rf["fwd"]
    _same(_triple(e.sw_pass(1, 0, q, t)), fwd, "mode 0")
    raw = e.sw_pass(1, 0, q, t, raw=True)
    over = fwd[:, 0] >= SW_PK_OVF
    assert np.array_equal(raw["score"] >= SW_PK_OVF, over), "the pairs flagged for the int32 re-run are the pairs at or above SW_PK_OVF"
    inside = ~over
    _same(raw["score"][inside], fwd[inside, 0], "raw mode 0 score")           # the partner of an overflowing pair included
    _same(raw["te"][inside], fwd[inside, 2], "raw mode 0 te")
    sure = inside & (raw["qe"] != -2)
    _same(raw["qe"][sure], fwd[sure, 1], "raw mode 0 qe")
    # one optimal cell by construction: never flagged; an optimum in every row: always (the partner of an overflowing pair may have either, it is compared above)
    assert (raw["qe"][C["kinds"] == "score-1-every-row"] == -2).all() and (raw["qe"][np.isin(C["kinds"], ("first-row", "score-1-one-cell"))] >= 0).all()
    assert (raw["qe"][inside] == -2).sum() < inside.sum() // 4


def check_reversed_query(e, C, Rf):
    q, t, rev = C["q"], C["t"], Rf["rev"]
    _same(e.sw_pass(1, 1, q, t)["score"], rev, "mode 1")
    raw = e.sw_pass(1, 1, q, t, raw=True)["score"]
    inside = rev < SW_PK_OVF
    _same(raw[inside], rev[inside], "raw mode 1")
    assert (raw[~inside] >= SW_PK_OVF).all() and (~inside).sum() == 2


def check_start(e, C, Rf):
    """MODE 2 on the forward ends (overflowing pairs included: re-run in int32) and on the hand-cut boxes"""
    q, t, fwd, pos = C["q"], C["t"], Rf["fwd"], Rf["pos"]
    ends = np.zeros((len(pos), 4), np.int32)
    ends[:, 1], ends[:, 3] = fwd[pos, 1], fwd[pos, 2]
    _same(_triple(e.sw_pass(1, 2, q[pos], t[pos], box=ends)), Rf["st"], "mode 2")
    b = C["boxes"]
    bx = np.zeros((len(b), 4), np.int32)
    bx[:, 1], bx[:, 3] = b[:, 2], b[:, 3]
    _same(_triple(e.sw_pass(1, 2, b[:, 0].astype(np.uint32), b[:, 1].astype(np.uint32), box=bx)), Rf["bst"], "mode 2, boxes")


def check_known(e, C, Rf, tab):
    """MODE 4 and MODE 6, raw (the packed kernel's own answers), table 1 or the wave-wide classes of table 3; known scores from 1 up"""
    q, t, fwd, pos, st = C["q"], C["t"], Rf["fwd"], Rf["pos"], Rf["st"]
    sel = fwd[pos, 0] < SW_PK_OVF
    ps = pos[sel]
    known = fwd[ps, 0].astype(np.int32)
    assert known.min() == 1
    _same(_triple(e.sw_pass(tab, 4, q[ps], t[ps], known=known, raw=True)), fwd[ps], ("mode 4", tab))
    ends = np.zeros((len(ps), 4), np.int32)
    ends[:, 1], ends[:, 3] = fwd[ps, 1], fwd[ps, 2]
    _same(_triple(e.sw_pass(tab, 6, q[ps], t[ps], box=ends, known=known, raw=True), True), st[sel], ("mode 6", tab))
    b, bst = C["boxes"], Rf["bst"]
    ok = bst[:, 0] > 0
    bx = np.zeros((int(ok.sum()), 4), np.int32)
    bx[:, 1], bx[:, 3] = b[ok, 2], b[ok, 3]
    r = e.sw_pass(tab, 6, b[ok, 0].astype(np.uint32), b[ok, 1].astype(np.uint32), box=bx, known=bst[ok, 0].astype(np.int32), raw=True)
    _same(_triple(r, True), bst[ok], ("mode 6, boxes", tab))


def check_all(e, C, Rf):
    """every check on one engine -> the class launches that took the two-task variant"""
    e.reset_stats()
    check_forward(e, C, Rf)
    check_reversed_query(e, C, Rf)
    check_start(e, C, Rf)
    check_known(e, C, Rf, 1)
    check_known(e, C, Rf, 3)
    return int(e.stats()["sw_multiquery_launches"])


def main():
    import unicore_amd as U
    from oracle import oracle_py as O
    C = build(O, sys.argv[1])
    launches = 0
    for gap in GAPS:
        Rf = references(O, C, gap)
        cases_are_what_they_claim(C, Rf)
        launches += check_all(engine(U, C, gap), C, Rf)
    print("multiquery_launches=%d" % launches)


if __name__ == "__main__":
    main()
