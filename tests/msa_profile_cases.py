"""Cases of rule UC-T/P shared by test_msa_profile.py (host twin) and test_msa_profile_gpu.py (HIP kernels).  A case is the keyword set of
unicore_amd.msa_profile_align: one or more groups, every group an MSA on two tracks (amino acids, 3Di) with the full rows behind it, the two
matrices and the gaps.  The MSAs are synthetic: rows descend from an ancestor as wide as the MSA, a deleted column is a gap, inserted residues
are in the row and not in the MSA - which is the state a star MSA leaves behind."""
import numpy as np

import matrix_cases as MC
import util

LETTERS = np.frombuffer((util.LET + "X").encode(), np.uint8)
GAP = ord("-")


def _rnd(rng, n):
    return rng.integers(0, 20, n, dtype=np.uint8), rng.integers(0, 20, n, dtype=np.uint8)


def descend(rng, anc, sub=0.2, indel=0.04):
    """one row from the ancestor (aa, 3di codes): -> (cells [2][W] bytes, residues [2][L] bytes)"""
    W = len(anc[0])
    cells, res = [np.full(W, GAP, np.uint8) for _ in range(2)], [[], []]
    for c in range(W):
        if rng.random() < indel:
            continue
        for t in range(2):
            x = int(rng.integers(0, 20)) if rng.random() < sub else int(anc[t][c])
            cells[t][c] = LETTERS[x]; res[t].append(LETTERS[x])
        if rng.random() < indel:
            k = int(rng.integers(1, 4))
            ins = _rnd(rng, k)
            for t in range(2):
                res[t].extend(LETTERS[ins[t]].tolist())
    return cells, [np.array(r, np.uint8) for r in res]


def window(rng, anc, L):
    """a row of exactly L residues: the ancestor's columns from a random start (mutated), random residues beyond the ancestor's end"""
    W = len(anc[0])
    start = int(rng.integers(0, max(W - L, 0) + 1))
    n = min(L, W - start)
    cells, res = [np.full(W, GAP, np.uint8) for _ in range(2)], []
    tail = _rnd(rng, L - n)
    for t in range(2):
        x = anc[t][start:start + n].copy()
        mut = rng.random(n) < 0.15
        x[mut] = rng.integers(0, 20, int(mut.sum()), dtype=np.uint8)
        cells[t][start:start + n] = LETTERS[x]
        res.append(np.concatenate([LETTERS[x], LETTERS[tail[t]]]))
    return cells, res


def case(groups, S3, SA, gap_open=10, gap_ext=1):
    go, width, res_off = [0], [], [0]
    cells, res = [[], []], [[], []]
    for rows in groups:
        go.append(go[-1] + len(rows)); width.append(len(rows[0][0][0]))
        for c, r in rows:
            assert len(c[0]) == width[-1] and len(r[0]) == len(r[1]) and ((c[0] == GAP) == (c[1] == GAP)).all()
            res_off.append(res_off[-1] + len(r[0]))
            for t in range(2):
                cells[t].append(np.asarray(c[t], np.uint8)); res[t].append(np.asarray(r[t], np.uint8))
    cat = lambda p: np.concatenate(p) if p else np.zeros(0, np.uint8)
    return dict(grp_off=np.array(go, np.uint64), width=np.array(width, np.uint32), cells=[cat(cells[0]), cat(cells[1])], res_off=np.array(res_off, np.uint64),
                res=[cat(res[0]), cat(res[1])], S3=np.asarray(S3, np.int8), SA=np.asarray(SA, np.int8), gap_open=gap_open, gap_ext=gap_ext)


def family(rng, W, m, **kw):
    anc = _rnd(rng, W)
    return [descend(rng, anc, **kw) for _ in range(m)]


def asymmetric(O):
    """the directed matrices of matrix_cases with entries at +48 and -48 on mirrored cells"""
    S3, SA = MC.matrices(O, "directed")
    S3, SA = S3.copy(), SA.copy()
    S3[0, 1], S3[1, 0], SA[2, 3], SA[3, 2] = 48, -48, -48, 48
    assert (S3 != S3.T).any() and (SA != SA.T).any() and max(abs(S3).max(), abs(SA).max()) == 48
    return S3, SA


def cases(O, chunk, cap=0):
    """{name: keyword set}.  chunk / cap: msa_profile_geometry()'s; widths sit one below, on and one above each of them"""
    S3, SA = MC.base(O)
    A3, AA = asymmetric(O)
    rng = np.random.default_rng(4711)
    out = {}
    for m in (2, 3, 8):                                                       # row counts
        out["rows_%d" % m] = case([family(rng, 90, m)], S3, SA)
    anc = _rnd(rng, 140)
    for L in (1, 2, 63, 64, 65, 257):                                         # row lengths, next to two ordinary rows
        out["length_%d" % L] = case([[descend(rng, anc), descend(rng, anc), window(rng, anc, L)]], S3, SA)
    widths = {1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1}
    if cap:
        widths |= {cap - 1, cap, cap + 1}
    for W in sorted(w for w in widths if w > 0):                              # widths: the chunk's edges, two chunks, the cap
        out["width_%d" % W] = case([family(rng, W, 3, indel=0.03)], S3, SA)
    out["many_groups"] = case([family(rng, int(rng.integers(5, 30)), 3) for _ in range(300)], S3, SA)      # several blocks of every launch
    out["rounding"] = case([family(rng, 70, 3, sub=0.5), family(rng, 70, 8, sub=0.5)], S3, SA)              # divisors 2 and 7
    out["asymmetric"] = case([family(rng, 80, 4), family(rng, 130, 3)], A3, AA)
    # ties: duplicate rows, and a row that repeats a motif so that end cells and paths tie
    fam = family(rng, 60, 2)
    motif = _rnd(rng, 6)
    rep = [np.tile(LETTERS[motif[t]], 8) for t in range(2)]
    repeat = ([np.concatenate([rep[t], np.full(12, GAP, np.uint8)]) for t in range(2)], [rep[t][:24] for t in range(2)])      # 48 motif columns, 24 residues
    out["ties"] = case([[fam[0], fam[0], fam[1], fam[1], repeat, repeat]], S3, SA)
    # gap bits: a row with 4 inserted residues and 3 deleted columns between conserved flanks
    anc = _rnd(rng, 100)
    base = [([LETTERS[anc[t]] for t in range(2)], [LETTERS[anc[t]] for t in range(2)]) for _ in range(3)]
    keep = np.r_[0:30, 33:100]
    extra = _rnd(rng, 4)
    r = [np.concatenate([LETTERS[anc[t][keep][:57]], LETTERS[extra[t]], LETTERS[anc[t][keep][57:]]]) for t in range(2)]
    c = [LETTERS[anc[t]].copy() for t in range(2)]
    for t in range(2):
        c[t][30:33] = GAP
    out["gap_bits"] = case([base + [(c, r)]], S3, SA)
    out["gap_bits_open_eq_ext"] = case([base + [(c, r)]], S3, SA, gap_open=3, gap_ext=3)
    # unaligned: under a matrix where W scores -5 against every letter a row of W never reaches a positive cell
    N3, NA = S3.copy(), SA.copy()
    for M in (N3, NA):
        M[18, :] = -5; M[:, 18] = -5
    fam = family(rng, 50, 3)
    wrow = ([np.full(50, GAP, np.uint8)] * 2, [np.full(17, ord("W"), np.uint8)] * 2)
    placed = ([np.concatenate([np.full(17, ord("W"), np.uint8), np.full(33, GAP, np.uint8)])] * 2, [np.full(17, ord("W"), np.uint8)] * 2)
    out["unaligned"] = case([fam + [wrow], fam + [placed]], N3, NA)
    # re-aligned: a family member that the MSA holds as a row of gaps
    anc = _rnd(rng, 75)
    fam = [descend(rng, anc) for _ in range(4)]
    lost = descend(rng, anc)
    out["realigned"] = case([fam + [([np.full(75, GAP, np.uint8)] * 2, lost[1])]], S3, SA)
    # a column without a residue between conserved halves: every row steps over it and the round drops it; a group of one row is left alone
    anc = _rnd(rng, 61)
    rows = []
    for _ in range(3):
        cc, rr = descend(rng, anc, indel=0.0, sub=0.05)
        cc = [np.concatenate([x[:30], [GAP], x[30:]]).astype(np.uint8) for x in cc]
        rows.append((cc, rr))
    out["empty_column_and_single"] = case([rows, family(rng, 20, 1), family(rng, 40, 2)], S3, SA)
    return out


def has_floor_case(kw):
    """True if a row of the case sees a negative numerator that its divisor does not divide: floor and truncation differ there"""
    import msa_profile_ref as R
    go, o = [int(x) for x in kw["grp_off"]], 0
    mats = [np.asarray(kw["SA"], np.int64).reshape(21, 21), np.asarray(kw["S3"], np.int64).reshape(21, 21)]
    for g in range(len(go) - 1):
        m, W = go[g + 1] - go[g], int(kw["width"][g])
        for t in range(2):
            grid = kw["cells"][t][o:o + m * W].reshape(m, W)
            num = np.zeros((W, 21), np.int64)
            for i in range(1, m):
                for c in range(W):
                    if grid[i, c] != GAP:
                        num[c] += mats[t][R.CODE[grid[i, c]]]
            if m > 2 and ((num < 0) & (num % (m - 1) != 0)).any():
                return True
        o += m * W
    return False
