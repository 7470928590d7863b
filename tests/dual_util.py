"""Inputs and the numpy reference for the two tie-break orders of the gapped DP (tests/test_dual_tiebreak.py, test_dual_tiebreak_gpu.py).

Among several optimal cells the spec reports the one in the first optimal column, then the first row (the FIRST answer).  The DP of the
mirror pair (t, q) is the transpose of the DP of (q, t) when both substitution matrices are symmetric, so the mirror's first answer is,
in the coordinates of (q, t), the optimal cell in the first optimal ROW, then the first column: the SECOND answer.  The two differ only
when optimal cells are anti-ordered (one lower and further left than the other), which random proteins almost never give: the pair kinds
here are built for ties."""
import numpy as np

from test_sw_kernels import CAPS, Dp, _mutate, _zero_partner

SW_PK_OVF = 0x7C00 - 256


def first_answer(H):
    """(score, row, col) of the optimal cell in the first optimal column, then the first row; (0, -1, -1) without a positive cell"""
    b = int(H.max())
    if b == 0:
        return 0, -1, -1
    j = int(np.nonzero(H.max(0) == b)[0][0])
    return b, int(np.nonzero(H[:, j] == b)[0][0]), j


def second_answer(H):
    """(score, row, col) of the optimal cell in the first optimal row, then the first column"""
    b = int(H.max())
    if b == 0:
        return 0, -1, -1
    i = int(np.nonzero(H.max(1) == b)[0][0])
    return b, i, int(np.nonzero(H[i] == b)[0][0])


def optimal_rows_cols(H):
    b = int(H.max())
    return (int((H.max(1) == b).sum()), int((H.max(0) == b).sum())) if b > 0 else (0, 0)


def _rnd(rng, n):
    return rng.integers(0, 20, n, dtype=np.uint8), rng.integers(0, 20, n, dtype=np.uint8)


def _cat(*parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _embed(rng, core, L):
    """core at a random offset of a random sequence of length L (the core alone if it does not fit)"""
    n = len(core[0])
    if n >= L:
        return core[0][:L].copy(), core[1][:L].copy()
    a = int(rng.integers(0, L - n + 1))
    return _cat(_rnd(rng, a), core, _rnd(rng, L - n - a))


def _lowc(rng, n, letters):
    """low-complexity stretch over two letters, the same in both tracks: many equal-scoring local alignments, in every direction"""
    x = rng.choice(np.asarray(letters, np.uint8), n)
    return x.copy(), x.copy()


def sweep_lengths(max_len=2048):
    """both edges and the middle of every packed class of tables 1 and 3"""
    Ls = set()
    for tab in (1, 3):
        lo = 1
        for cap in CAPS[tab]:
            Ls |= {lo, (lo + cap) // 2, cap}
            lo = cap + 1
    return sorted(x for x in Ls if x <= max_len)


def tie_pairs(seed, lengths, dp):
    """(s3, sa, pairs [(q, t)], kinds): per query length several targets built for tied optima, and plain ones.
      lowc      q and t hold independent low-complexity stretches over the same two letters: tied optimal cells all over, anti-ordered ones too
      crossed   q = .. A X rev(A) .., t = rev(A) Y A: two optimal alignments of equal score whose end cells are anti-ordered
      forked    q = .. A rev(A) M .., t = rev(A) A M: two optimal alignments END in one cell (M on M, then a gap over one copy and the other copy
                matched) and start in anti-ordered cells: the start pass's tie
      tandem    q = .. U U U .., t = U U: two optimal rows in one column (for the mirror: two columns in one row)
      zero-end / zero-start   the last / first residue pair scores 0: two optimal cells on one diagonal
      mutated   a plain homologue, in general one optimal cell"""
    rng = np.random.default_rng(seed)
    s3, sa, pairs, kinds = [], [], [], []

    def add(x):
        s3.append(np.ascontiguousarray(x[0], np.uint8)); sa.append(np.ascontiguousarray(x[1], np.uint8))
        return len(s3) - 1

    for L in lengths:
        for rep in range(3):
            letters = rng.choice(20, 2, replace=False)
            nq = int(rng.integers(16, 49))
            q = add(_embed(rng, _lowc(rng, nq, letters), L))
            tcore = _lowc(rng, int(rng.integers(12, 41)), letters)
            t = add(_cat(_rnd(rng, int(rng.integers(0, 9))), tcore, _rnd(rng, int(rng.integers(0, 9)))))
            pairs.append((q, t)); kinds.append("lowc")
        n = 12 if L >= 40 else max(2, L // 3)
        for rep in range(2):
            A = _rnd(rng, n)
            rA = (A[0][::-1].copy(), A[1][::-1].copy())
            X, Y = _rnd(rng, int(rng.integers(3, 9))), _rnd(rng, int(rng.integers(3, 9)))
            q = add(_embed(rng, _cat(A, X, rA), L))
            pairs.append((q, add(_cat(rA, Y, A)))); kinds.append("crossed")
            M = _rnd(rng, 2 * n)
            q = add(_embed(rng, _cat(A, rA, M), L))
            pairs.append((q, add(_cat(rA, A, M)))); kinds.append("forked")
        U = _rnd(rng, n)
        q = add(_embed(rng, _cat(U, U, U), L))
        pairs.append((q, add(_cat(U, U)))); kinds.append("tandem")
        q3, qa = _rnd(rng, L)
        q = add((q3, qa))
        if L >= 3:
            y3, ya = _zero_partner(dp.S3, dp.SA, q3[-1], qa[-1], rng)
            a = max(0, L - 60)                     # a copy of the query's tail (short targets keep the numpy DP cheap)
            pairs.append((q, add((np.append(q3[a:-1], y3), np.append(qa[a:-1], ya))))); kinds.append("zero-end")
            y3, ya = _zero_partner(dp.S3, dp.SA, q3[0], qa[0], rng)
            pairs.append((q, add((np.insert(q3[1:60], 0, y3), np.insert(qa[1:60], 0, ya))))); kinds.append("zero-start")
        a = int(rng.integers(0, max(1, L - 80)))
        pairs.append((q, add(_mutate(rng, q3[a:a + 80], qa[a:a + 80], 0.1, indels=False)))); kinds.append("mutated")
    return s3, sa, pairs, np.array(kinds)


def reference(dp, s3, sa, q, t):
    """forward DP and start-pass DP (on the reversed prefixes up to the forward pass's first answer) of the pair (q, t):
    dict(fwd1, fwd2 = (score, qe, te) first / second answer, rows, cols = optimal rows / columns of the forward DP,
         st1, st2 = first / second answer of the start pass, srows = its optimal rows)"""
    H = dp.H(s3[q], sa[q], s3[t], sa[t])
    f1, f2 = first_answer(H), second_answer(H)
    r = dict(fwd1=f1, fwd2=f2, rows=optimal_rows_cols(H)[0], cols=optimal_rows_cols(H)[1])
    if f1[0] > 0:
        r.update(start_reference(dp, s3, sa, q, t, f1[1], f1[2]))
    return r


def start_reference(dp, s3, sa, q, t, qe, te):
    """the start pass of (q, t) from the end cell (qe, te): DP of reverse(q[0..qe]) x reverse(t[0..te])"""
    Hs = dp.H(s3[q][qe::-1], sa[q][qe::-1], s3[t][te::-1], sa[t][te::-1])
    return dict(st1=first_answer(Hs), st2=second_answer(Hs), srows=optimal_rows_cols(Hs)[0])
