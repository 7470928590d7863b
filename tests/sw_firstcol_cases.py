"""Cases and checks of tests/test_sw_firstcol_gpu.py: what the packed gapped kernels (uc_sw_pk_impl.hpp) report as the FIRST optimal column, tracked on one
packed register (the age of the maximum, MODE 0 / 2), and the target letters of the G = 16 / 32 classes, two columns per 32-bit load (every mode but 7) -
one pass at a time through Engine.sw_pass, raw and not raw, against the scalar oracle: scores exact, te the oracle's first optimal column wherever the
score is positive, qe the oracle's row (raw: or -2, the flag of an ambiguous end row).  Default matrices and gaps.

Queries: two per class of table 1, of 20 (16, 2), 180 (16, 12), 420 (32, 14) and 800 residues (64, 14): a random one and a crafted one.

The random query's targets (its pair list has 11 entries, an ODD number: the last slot has no B half):
  lengths 1, 2, 3 (copies of its first residues) and 16, 17, 255, 256 (random, a mutated window of the query inside): the slot (256, 255) differs by 1;
  32,769 and 65,535 residues, random, a copy of a query window as their LAST residues: an end column with bit 15 set, the optimum in the last column,
      and at G = 64 more than 65,536 steps (nst = 65,535 + 64 rounded up);
  `inner`: a copy of a query window, a multiple of 16 residues long (so that exactly the 16 PAD entries of the device layout separate it from its
      neighbours); the sequence in front of it in the database ends with the residues that precede the window in the query and the one behind it
      starts with those that follow it - a read past either end would lengthen the match and raise the score;
  `tail`: a copy of the query's last two residues, i.e. of the first two of the reversed query (MODE 1).
The first and the last sequence of the database are targets (the random 256 of the first class, the crafted `last-column` of the last).

The crafted query is one filler letter y except rows (k1, k1 + 1) = (a, b) in lane 1 and (k2, k2 + 1) = (b, a) in the last lane that holds two rows
(a, b, y and the targets' filler w score negative against each other): a diagonal "ab" or "ba" scores S = s(a, a) + s(b, b), the optimum.  Its targets:
  `low-lane-first`   ab www ba w     optimal cells (k1 + 1, 1) and (k2 + 1, 6): two lanes, the lower lane holds the smaller column
  `high-lane-first`  ba www ab w     optimal cells (k2 + 1, 1) and (k1 + 1, 6): the higher lane does, and it reaches that column in a LATER step than
                                     the lower lane reaches its own (step = column + lane): the column decides, not the step
  `one-lane-twice`   w ab ww ab ww   optimal cells (k1 + 1, 2) and (k1 + 1, 6): one lane, one row, two columns - the first stays
  `far`              w x 200, ab, w x 7   the slot partner of `one-lane-twice`, 200 residues longer
  `column-0`         a wwww          the optimum s(a, a) in column 0, rows k1 and k2 + 1
  `last-column`      wwww a          ... in the last column
cases_are_what_they_claim() asserts all of this from the oracle and from a full-matrix DP (tests/sw_dp.py), and the slots from the planner's order
(a query's pairs by target length, longest first, ties in list order; a slot = two neighbours).

Run as a program (argv: unused) it builds the same cases and runs every check in a process of its own: UC_SW_TASK_QUERIES is read once per process.
Prints `multiquery_launches=N`."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")

import matrix_cases as MC      # noqa: E402
import sw_dp                   # noqa: E402
import util                    # noqa: E402

SW_PK_OVF = 0x7C00 - 256
TE_UNIQUE = 1 << 30
OPTIONS = "-c 0.8"
# query length -> (index in class table 1, G, R): caps 32, 64, ... 384 in steps of 32 (G = 16), 448 ... 768 in steps of 64 (G = 32), 896 ... (G = 64)
CLASSES = {20: (0, 16, 2), 180: (5, 16, 12), 420: (12, 32, 14), 800: (18, 64, 14)}
SHORT = (1, 2, 3, 16, 17, 255, 256)
LONG = (32769, 65535)


def letters(O):
    """a, b, y, w: every pair among them scores negative, a and b score positive against themselves"""
    S3, SA = MC.base(O)
    tot = (S3 + SA)[:20, :20]
    neg = lambda u, v: tot[u, v] < 0 and tot[v, u] < 0
    for a in np.argsort(-np.diag(tot)):
        pick = [int(a)]
        for c in range(20):
            if c != a and all(neg(c, d) for d in pick):
                pick.append(c)
            if len(pick) == 4:
                return dict(zip("abyw", pick)), tot
    raise AssertionError("no four mutually negative letters")


def build(O):
    L, tot = letters(O)
    a, b, y, w = (np.uint8(L[k]) for k in "abyw")
    assert tot[a, a] > 0 and tot[b, b] > 0
    rng = np.random.default_rng(777)
    s3, sa, pairs, kinds = [], [], [], []

    def add(x3, xa=None):
        x3 = np.ascontiguousarray(x3, np.uint8)
        s3.append(x3); sa.append(x3.copy() if xa is None else np.ascontiguousarray(xa, np.uint8))
        return len(s3) - 1

    def rnd(n):
        return rng.integers(0, 20, n, dtype=np.uint8), rng.integers(0, 20, n, dtype=np.uint8)

    def cat(*parts):
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def mutated(x3, xa, rate=0.1):
        x3, xa = x3.copy(), xa.copy()
        for x in (x3, xa):
            m = rng.random(len(x)) < rate
            x[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
        return x3, xa

    def pair(q, t, kind):
        pairs.append((q, t)); kinds.append(kind)

    rep = lambda c, n: np.full(n, c, np.uint8)
    crafted = {}
    qr = {n: rnd(n) for n in CLASSES}                      # the random queries' residues (added to the database further down)
    for n, (_, G, R) in CLASSES.items():
        q3, qa = qr[n]
        # the first sequence of the database is the first class's 256-residue target
        t256 = add(*cat(rnd(60), mutated(q3[: min(n, 140)], qa[: min(n, 140)]), rnd(256 - 60 - min(n, 140))))
        q = add(q3, qa)
        pair(q, t256, "len-256")
        for m in SHORT[:-1]:
            if m <= 3:
                t = add(q3[:m], qa[:m])
            else:
                win = min(m, n, 140)
                at = int(rng.integers(0, m - win + 1))
                t = add(*cat(rnd(at), mutated(q3[:win], qa[:win]), rnd(m - win - at)))
            pair(q, t, "len-%d" % m)
        for m in LONG:
            win = min(n, 100)
            k = (n - win) // 2
            pair(q, add(*cat(rnd(m - win), (q3[k:k + win], qa[k:k + win]))), "long-%d" % m)
        win, k = 16, min(n // 3, n - 18)
        add(*cat(rnd(20), (q3[max(k - 30, 0):k], qa[max(k - 30, 0):k])))                       # in front: ends with what precedes the window
        pair(q, add(q3[k:k + win], qa[k:k + win]), "inner")
        add(*cat((q3[k + win:k + win + 30], qa[k + win:k + win + 30]), rnd(20)))              # behind: starts with what follows it
        pair(q, add(q3[n - 2:], qa[n - 2:]), "tail")
        # the crafted query and its targets
        k1, k2 = R, R * ((n - 2) // R)
        assert k1 // R != k2 // R and (k2 + 1) // R == k2 // R and k2 + 1 < n
        c = rep(y, n)
        c[k1], c[k1 + 1], c[k2], c[k2 + 1] = a, b, b, a
        qc = add(c)
        crafted[qc] = (k1, k2)
        ab, ba = np.array([a, b], np.uint8), np.array([b, a], np.uint8)
        pair(qc, add(np.concatenate([ab, rep(w, 3), ba, rep(w, 1)])), "low-lane-first")
        pair(qc, add(np.concatenate([ba, rep(w, 3), ab, rep(w, 1)])), "high-lane-first")
        pair(qc, add(np.concatenate([rep(w, 1), ab, rep(w, 2), ab, rep(w, 2)])), "one-lane-twice")
        pair(qc, add(np.concatenate([rep(w, 200), ab, rep(w, 7)])), "far")
        pair(qc, add(np.concatenate([rep(a, 1), rep(w, 4)])), "column-0")
        pair(qc, add(np.concatenate([rep(w, 4), rep(a, 1)])), "last-column")
    lens = np.array([len(x) for x in s3])
    return dict(s3=s3, sa=sa, lens=lens, kinds=np.array(kinds), q=np.array([u for u, _ in pairs], np.uint32), t=np.array([v for _, v in pairs], np.uint32),
                crafted=crafted, S=int(tot[a, a] + tot[b, b]), Sa=int(tot[a, a]))


def references(O, C):
    """the oracle's answers: forward (score, qe, te), the reversed-query score, the start pass on the forward ends"""
    p = util.oracle_params(O, OPTIONS)
    s3, sa, q, t = C["s3"], C["sa"], C["q"], C["t"]
    n = len(q)
    fwd = np.array([O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p) for i in range(n)], np.int64).reshape(n, 3)
    rev = np.array([O.sw(s3[q[i]], sa[q[i]], s3[t[i]], sa[t[i]], p, rev_q=1)[0] for i in range(n)], np.int64)
    pos = np.nonzero(fwd[:, 0] > 0)[0]
    st = np.array([O.sw(s3[q[i]][: fwd[i, 1] + 1], sa[q[i]][: fwd[i, 1] + 1], s3[t[i]][: fwd[i, 2] + 1], sa[t[i]][: fwd[i, 2] + 1], p, rev_q=1, rev_t=1)
                   for i in pos], np.int64).reshape(len(pos), 3)
    return dict(p=p, fwd=fwd, rev=rev, pos=pos, st=st)


def slots(C, idx):
    """the planner's slots of one query's pairs `idx` (list order): by target length, longest first, ties in list order; two neighbours a slot"""
    order = idx[np.argsort(-C["lens"][C["t"][idx]], kind="stable")]
    return [tuple(order[i:i + 2]) for i in range(0, len(order), 2)]


def cases_are_what_they_claim(C, Rf):
    fwd, kinds, q, t, lens = Rf["fwd"], C["kinds"], C["q"], C["t"], C["lens"]
    assert (fwd[:, 0] > 0).all() and (fwd[:, 0] < SW_PK_OVF).all() and (Rf["rev"] < SW_PK_OVF).all()
    assert 0 in t and len(lens) - 1 in t, "the first and the last sequence of the database are targets"
    assert sorted(set(lens[q].tolist())) == sorted(CLASSES)
    dp = sw_dp.Dp(Rf["p"])
    diffs, odd = set(), 0
    for qq in np.unique(q):
        idx = np.nonzero(q == qq)[0]
        assert len(idx) <= 48, "one task per query in every class"
        sl = slots(C, idx)
        odd += len(sl[-1]) == 1
        diffs |= {int(lens[t[s[0]]] - lens[t[s[1]]]) for s in sl if len(s) == 2}
        if qq in C["crafted"]:
            k1, k2 = C["crafted"][qq]
            S, Sa = C["S"], C["Sa"]
            want = {"low-lane-first": (S, {(k1 + 1, 1), (k2 + 1, 6)}), "high-lane-first": (S, {(k2 + 1, 1), (k1 + 1, 6)}),
                    "one-lane-twice": (S, {(k1 + 1, 2), (k1 + 1, 6)}), "far": (S, {(k1 + 1, 201)}),
                    "column-0": (Sa, {(k1, 0), (k2 + 1, 0)}), "last-column": (Sa, {(k1, 4), (k2 + 1, 4)})}
            for i in idx:
                H = dp.H(C["s3"][qq], C["sa"][qq], C["s3"][t[i]], C["sa"][t[i]])
                score, cells = want[kinds[i]]
                assert H.max() == score == fwd[i, 0], (kinds[i], int(H.max()), score)
                assert {(int(r), int(c)) for r, c in zip(*np.nonzero(H == score))} == cells, kinds[i]
                assert fwd[i, 2] == min(c for _, c in cells) and fwd[i, 1] == min(r for r, c in cells if c == fwd[i, 2])
            far, twice = idx[kinds[idx] == "far"][0], idx[kinds[idx] == "one-lane-twice"][0]
            assert (far, twice) in sl, "`far` and `one-lane-twice` share a slot"
        else:
            (i256,), (i255,) = idx[kinds[idx] == "len-256"], idx[kinds[idx] == "len-255"]
            assert (i256, i255) in sl
            for m in LONG:
                (i,) = idx[kinds[idx] == "long-%d" % m]
                assert fwd[i, 2] == m - 1, "the optimum of a long target ends in its last column"
            (i,) = idx[kinds[idx] == "inner"]
            assert fwd[i, 2] == lens[t[i]] - 1 and lens[t[i]] % 16 == 0      # the whole window matches; a longer read would go on matching
            n, win = int(lens[qq]), int(lens[t[i]])
            k, front, behind = min(n // 3, n - 18), t[i] - 1, t[i] + 1
            assert np.array_equal(C["s3"][front][-min(k, 30):], C["s3"][qq][k - min(k, 30):k]) and np.array_equal(C["s3"][behind][:2], C["s3"][qq][k + win:k + win + 2])
    assert 1 in diffs and 200 in diffs and odd >= 4, (sorted(diffs), odd)


def engine(U, C):
    e = U.Engine(OPTIONS, verbosity=1)
    e.set_db(*util.flat(C["s3"], C["sa"]))
    return e


def _triple(r, mask_unique=False):
    te = np.where(r["te"] >= 0, r["te"] & ~TE_UNIQUE, r["te"]) if mask_unique else r["te"]
    return np.stack([r["score"], r["qe"], te], 1)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.nonzero((got != want).reshape(len(want), -1).any(1))[0]
    assert not len(bad), (what, bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())


def _raw_ends(raw, want, what):
    """a raw tracking pass: the score exact, te the first optimal column, qe the oracle's row or the flag -2"""
    _same(raw["score"], want[:, 0], what + " score")
    _same(raw["te"], want[:, 2], what + " te")
    sure = raw["qe"] != -2
    _same(raw["qe"][sure], want[sure, 1], what + " qe")
    return sure


def check_forward(e, C, Rf):
    q, t, fwd, kinds = C["q"], C["t"], Rf["fwd"], C["kinds"]
    r = e.sw_pass(1, 0, q, t)
    _same(r["cls"], [CLASSES[int(n)][0] for n in C["lens"][q]], "class of the query length")
    _same(_triple(r), fwd, "mode 0")
    raw = e.sw_pass(1, 0, q, t, raw=True)
    sure = _raw_ends(raw, fwd, "raw mode 0")
    # one row holds every optimal cell of these: never flagged; two rows hold one each: always
    assert sure[np.isin(kinds, ("one-lane-twice", "far"))].all()
    assert not sure[np.isin(kinds, ("low-lane-first", "high-lane-first", "column-0", "last-column"))].any()


def check_reversed_query(e, C, Rf):
    q, t = C["q"], C["t"]
    _same(e.sw_pass(1, 1, q, t)["score"], Rf["rev"], "mode 1")
    _same(e.sw_pass(1, 1, q, t, raw=True)["score"], Rf["rev"], "raw mode 1")


def _ends(fwd):
    ends = np.zeros((len(fwd), 4), np.int32)
    ends[:, 1], ends[:, 3] = fwd[:, 1], fwd[:, 2]
    return ends


def check_start(e, C, Rf):
    """MODE 2: the reversed target, read downwards from the forward end column onto the PAD entries in front of the sequence"""
    q, t, fwd, st = C["q"], C["t"], Rf["fwd"], Rf["st"]
    assert len(Rf["pos"]) == len(q)
    _same(_triple(e.sw_pass(1, 2, q, t, box=_ends(fwd))), st, "mode 2")
    _raw_ends(e.sw_pass(1, 2, q, t, box=_ends(fwd), raw=True), st, "raw mode 2")


def check_known(e, C, Rf):
    """MODE 4 and MODE 6, raw: the letter path of the known-score kernels, forward and reversed target"""
    q, t, fwd, st = C["q"], C["t"], Rf["fwd"], Rf["st"]
    known = fwd[:, 0].astype(np.int32)
    _same(_triple(e.sw_pass(1, 4, q, t, known=known, raw=True)), fwd, "mode 4")
    _same(_triple(e.sw_pass(1, 6, q, t, box=_ends(fwd), known=known, raw=True), True), st, "mode 6")


def check_all(e, C, Rf):
    """every check on one engine -> the class launches that took the two-task variant"""
    e.reset_stats()
    check_forward(e, C, Rf)
    check_reversed_query(e, C, Rf)
    check_start(e, C, Rf)
    check_known(e, C, Rf)
    return int(e.stats()["sw_multiquery_launches"])


def main():
    import unicore_amd as U
    from oracle import oracle_py as O
    C = build(O)
    Rf = references(O, C)
    cases_are_what_they_claim(C, Rf)
    print("multiquery_launches=%d" % check_all(engine(U, C), C, Rf))


if __name__ == "__main__":
    main()
