"""Test-side restatement of the oracle's traceback() (oracle/uc_oracle.c, spec UC-1.1 / E6) that also returns the PATH.

The oracle returns (alignment length, identities, gap opens) of the box; the backtrace tests need the operations.  Same rule, in
numpy row sweeps + a scalar walk:  from the box's end cell, diagonal if H(i,j) = H(i-1,j-1) + s(i,j), else the F gap (consumes a query
residue, `I`) if H = F, else the E gap (consumes a target residue, `D`); a gap is left as soon as it can be; stop at H = 0 or at the edge."""
import re

import numpy as np

NEG = -(1 << 28)


def matrices(p):
    return np.array(p.S3[:], np.int32).reshape(21, 21), np.array(p.SA[:], np.int32).reshape(21, 21)


def dp(S, gap_open, gap_ext):
    """H, E, F of the box with the oracle's borders (H = 0, E = F = NEG on row / column 0), shape (lq + 1, lt + 1)"""
    assert gap_open >= gap_ext >= 0       # E of a row from the row's H before its own horizontal gaps is exact then
    lq, lt = S.shape
    H = np.zeros((lq + 1, lt + 1), np.int32)
    E = np.full((lq + 1, lt + 1), NEG, np.int32)
    F = np.full((lq + 1, lt + 1), NEG, np.int32)
    ar = np.arange(lt + 1, dtype=np.int32) * gap_ext
    for i in range(1, lq + 1):
        F[i, 1:] = np.maximum(F[i - 1, 1:] - gap_ext, H[i - 1, 1:] - gap_open)
        h = np.maximum(np.maximum(H[i - 1, :-1] + S[i - 1], F[i, 1:]), 0)
        m = np.maximum.accumulate(np.concatenate(([0], h)) + ar)
        E[i, 1:] = m[:-1] - gap_open - ar[1:] + gap_ext
        H[i, 1:] = np.maximum(h, E[i, 1:])
    return H, E, F


def rle(ops):
    out, k = [], 0
    while k < len(ops):
        j = k
        while j < len(ops) and ops[j] == ops[k]:
            j += 1
        out.append("%d%s" % (j - k, ops[k]))
        k = j
    return "".join(out)


def traceback(q3, qa, t3, ta, S3, SA, gap_open, gap_ext):
    """(aln_len, idents, gap_opens, cigar, H of the end cell) of the box that the four code arrays span"""
    S = S3[q3][:, t3] + SA[qa][:, ta]
    H, E, F = dp(S, gap_open, gap_ext)
    i, j = S.shape
    state, ln, idn, gaps, ops = 0, 0, 0, 0, []
    while i > 0 and j > 0:
        if state == 0:
            h = H[i, j]
            if h == 0:
                break
            if h == H[i - 1, j - 1] + S[i - 1, j - 1]:
                ln += 1; idn += int(qa[i - 1] == ta[j - 1]); i -= 1; j -= 1
                ops.append("M")
            elif h == F[i, j]:
                state = 1; gaps += 1
            else:
                state = 2; gaps += 1
        elif state == 1:
            ln += 1
            ops.append("I")
            if F[i, j] == H[i - 1, j] - gap_open:
                state = 0
            i -= 1
        else:
            ln += 1
            ops.append("D")
            if E[i, j] == H[i, j - 1] - gap_open:
                state = 0
            j -= 1
    return ln, idn, gaps, rle(ops[::-1]), int(H[S.shape[0], S.shape[1]])


def parse(cigar):
    runs = [(int(n), op) for n, op in re.findall(r"(\d+)([MID])", cigar)]
    assert "".join("%d%s" % r for r in runs) == cigar, cigar
    return runs


def swap_id(cigar):
    return cigar.translate(str.maketrans("ID", "DI"))


def check_valid(cigar, q3, qa, t3, ta, S3, SA, gap_open, gap_ext, aln_len, idents, gap_opens, score):
    """every point of the validity list: q*, t* are the residues of the box [qStart..qEnd] x [tStart..tEnd]"""
    runs = parse(cigar)
    assert all(n > 0 for n, _ in runs)
    assert all(a[1] != b[1] for a, b in zip(runs, runs[1:])), cigar          # adjacent runs never share a letter
    cnt = {op: sum(n for n, o in runs if o == op) for op in "MID"}
    assert sum(cnt.values()) == aln_len, (cigar, aln_len)
    assert cnt["M"] + cnt["I"] == len(q3) and cnt["M"] + cnt["D"] == len(t3), (cigar, len(q3), len(t3))
    assert sum(1 for _, o in runs if o != "M") == gap_opens, (cigar, gap_opens)
    i = j = idn = sc = 0
    for n, op in runs:
        if op == "M":
            sc += int((S3[q3[i:i + n], t3[j:j + n]] + SA[qa[i:i + n], ta[j:j + n]]).sum())
            idn += int((qa[i:i + n] == ta[j:j + n]).sum())
            i += n; j += n
        else:
            sc -= gap_open + (n - 1) * gap_ext
            if op == "I":
                i += n
            else:
                j += n
    assert idn == idents, (cigar, idn, idents)
    assert sc == score, (cigar, sc, score)                                   # the path is optimal: its score is the box's score


# ---- pair material shared by the CPU and the GPU tests --------------------------------------------------------------------
def _rnd(rng, n):
    return rng.integers(0, 20, n, dtype=np.uint8), rng.integers(0, 20, n, dtype=np.uint8)


def mutate(rng, a3, aa, rate):
    """a copy with substitutions, one deletion of 3 and one insertion of 4 residues"""
    b3, ba = a3.copy(), aa.copy()
    m = rng.random(len(b3)) < rate
    b3[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
    m = rng.random(len(ba)) < rate
    ba[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
    if len(b3) > 40:
        c = int(rng.integers(10, len(b3) // 2))
        b3, ba = np.delete(b3, slice(c, c + 3)), np.delete(ba, slice(c, c + 3))
        c = int(rng.integers(len(b3) // 2, len(b3) - 10))
        i3, ia = _rnd(rng, 4)
        b3, ba = np.concatenate([b3[:c], i3, b3[c:]]), np.concatenate([ba[:c], ia, ba[c:]])
    return b3, ba


def zigzag(rng, L):
    """q = A X B, t = A Y B with unrelated X, Y (the construction tests/test_sw_kernels.py uses for band misses)"""
    lx, ly = int(rng.integers(8, 40)), int(rng.integers(8, 40))
    l1 = int(rng.integers(40, L - lx - 40))
    a, x, b, y = _rnd(rng, l1), _rnd(rng, lx), _rnd(rng, L - l1 - lx), _rnd(rng, ly)
    return (np.concatenate([a[0], x[0], b[0]]), np.concatenate([a[1], x[1], b[1]])), \
           (np.concatenate([a[0], y[0], b[0]]), np.concatenate([a[1], y[1], b[1]]))


def pair_set(rng, lengths, per_length=1):
    """sequences + (q, t, kind) triples: mutated copies with indels, zig-zag pairs, unrelated pairs, for every length"""
    s3, sa, pairs = [], [], []

    def add(x):
        s3.append(x[0]); sa.append(x[1])
        return len(s3) - 1
    for L in lengths:
        for _ in range(per_length):
            a = _rnd(rng, L)
            qi = add(a)
            pairs.append((qi, add(mutate(rng, a[0], a[1], 0.15)), "mutated"))
            if L >= 140:
                z = zigzag(rng, L)
                pairs.append((add(z[0]), add(z[1]), "zigzag"))
            pairs.append((qi, add(_rnd(rng, max(1, L // 2 + 3))), "unrelated"))
    return s3, sa, pairs


def box_of(O, p, q3, qa, t3, ta):
    """(score, qs, qe, ts, te) as the engine finds them: forward pass, then the reversed prefixes"""
    s, qe, te = O.sw(q3, qa, t3, ta, p)
    if s <= 0:
        return None
    s2, dq, dt = O.sw(q3[: qe + 1], qa[: qe + 1], t3[: te + 1], ta[: te + 1], p, rev_q=1, rev_t=1)
    assert s2 == s
    return s, qe - dq, qe, te - dt, te
