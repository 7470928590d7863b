"""Test-side restatement of rule UC-T/G (`unicore tree -a progressive`) in plain Python and numpy: the guide-tree distances and the merge
order over nj_ref.join, the profile-profile merge (column counts, the floor-divided cell score, the overlap DP without a floor, the end cell on the last
row or column, one walk with E6's preferences, the merged columns) and the progressive MSA along a merge list.  Track 0 is the amino acids, track 1 the
3Di letters; the matrices are [column letter][row letter], side a giving the column letter.  No product code is involved."""
import numpy as np

import nj_ref

GAP = ord("-")
LET = "ACDEFGHIKLMNPQRSTVWY"
CODE = np.full(256, 20, np.uint8)
for _k, _c in enumerate(LET):
    CODE[ord(_c)] = CODE[ord(_c.lower())] = _k
NEG = -(1 << 28)
MAX_ROWS = 8192


def self_score(res, mats):
    """res: [aa, 3di] bytes of one row; mats: [SA, S3]"""
    return sum(int(mats[t][CODE[c], CODE[c]]) for t in range(2) for c in np.asarray(res[t], np.uint8))


def distances(tri, selfs):
    """D [m][m] as a list of lists from the packed triangle (row i as query) and the self scores"""
    m = len(selfs)
    D = [[0.0] * m for _ in range(m)]
    k = 0
    for i in range(m):
        for j in range(i + 1, m):
            den = min(int(selfs[i]), int(selfs[j]))
            d = 1.0 if den <= 0 else 1.0 - float(int(tri[k])) / float(den)
            if d < 0.0:
                d = 0.0
            D[i][j] = D[j][i] = d
            k += 1
    return D


def merge_list(D):
    """[(a, b)] in merge order; merge k creates node m + k"""
    m = len(D)
    if m == 1:
        return []
    if m == 2:
        return [(0, 1)]
    j = nj_ref.join(D)
    out = [(int(a), int(b)) for a, b in zip(j["join_a"], j["join_b"])]
    r = [int(x) for x in j["root_node"]]
    out.append((r[0], r[1]))
    out.append((m + len(out) - 1, r[2]))
    return out


def guide(tri, selfs):
    D = distances(tri, selfs)
    return D, merge_list(D)


def counts(grid):
    """cnt [W][21] of one track of a node: grid [m][W] bytes"""
    m, W = grid.shape
    c = np.zeros((W, 21), np.int64)
    for i in range(m):
        for k in range(W):
            if grid[i, k] != GAP:
                c[k, CODE[grid[i, k]]] += 1
    return c


def cell_scores(a, b, mats):
    """s [Wa][Wb]: a, b are [aa grid, 3di grid]; Python's // is the floor"""
    ma, mb = a[0].shape[0], b[0].shape[0]
    raw = sum(counts(a[t]) @ np.asarray(mats[t], np.int64).reshape(21, 21) @ counts(b[t]).T for t in range(2))
    return raw // (ma * mb)


def dp(s, gap_open, gap_ext):
    """H, E, F [(Wa + 1)][(Wb + 1)] of the overlap alignment without a floor.  A row at a time: E along the row is a running maximum, which gives the
    recurrence's own values because open >= ext (an E opened from a cell that E itself set never beats the extension)."""
    Wa, Wb = s.shape
    H = np.zeros((Wa + 1, Wb + 1), np.int64)
    E = np.full((Wa + 1, Wb + 1), NEG, np.int64)
    F = np.full((Wa + 1, Wb + 1), NEG, np.int64)
    jj = np.arange(Wb + 1, dtype=np.int64)
    for i in range(1, Wa + 1):
        F[i, 1:] = np.maximum(H[i - 1, 1:] - gap_open, F[i - 1, 1:] - gap_ext)
        G = np.empty(Wb + 1, np.int64)
        G[0] = 0
        G[1:] = np.maximum(H[i - 1, :-1] + s[i - 1], F[i, 1:])
        run = np.maximum.accumulate(G + jj * gap_ext)            # max over k <= j of G(k) + k ext
        E[i, 1:] = run[:-1] - gap_open - jj[:-1] * gap_ext       # E(j) = max over k < j of G(k) - open - (j - 1 - k) ext
        H[i, 1:] = np.maximum(G[1:], E[i, 1:])
    return H, E, F


def dp_plain(s, gap_open, gap_ext):
    """the recurrence cell by cell, as the rule states it (the tests compare dp against it on small cases)"""
    Wa, Wb = s.shape
    H = [[0] * (Wb + 1) for _ in range(Wa + 1)]
    E = [[NEG] * (Wb + 1) for _ in range(Wa + 1)]
    F = [[NEG] * (Wb + 1) for _ in range(Wa + 1)]
    for i in range(1, Wa + 1):
        for j in range(1, Wb + 1):
            F[i][j] = max(H[i - 1][j] - gap_open, F[i - 1][j] - gap_ext)
            E[i][j] = max(H[i][j - 1] - gap_open, E[i][j - 1] - gap_ext)
            H[i][j] = max(H[i - 1][j - 1] + int(s[i - 1, j - 1]), F[i][j], E[i][j])
    return np.array(H, np.int64), np.array(E, np.int64), np.array(F, np.int64)


def merge(a, b, mats, gap_open, gap_ext):
    """a, b: [aa grid, 3di grid] (m x W uint8).  Returns a dict: score, is, js, ie, je, runs, width, cells [aa grid, 3di grid]"""
    (ma, Wa), (mb, Wb) = a[0].shape, b[0].shape
    if Wa == 0 or Wb == 0:
        sc, i0, j0, ie, je, runs = 0, 0, 0, 0, 0, []
    else:
        s = cell_scores(a, b, mats)
        H, E, F = dp(s, gap_open, gap_ext)
        cand = [(int(H[Wa, j]), -j, -Wa) for j in range(Wb + 1)] + [(int(H[i, Wb]), -Wb, -i) for i in range(Wa + 1)]
        sc, nj, ni = max(cand)
        ie, je = -ni, -nj
        i, j, state, ops = ie, je, 0, []
        while i > 0 and j > 0:
            if state == 0:
                h = H[i, j]
                if h == H[i - 1, j - 1] + s[i - 1, j - 1]:
                    ops.append(0); i -= 1; j -= 1
                elif h == F[i, j]:
                    state = 1
                else:
                    assert h == E[i, j]
                    state = 2
            elif state == 1:
                ops.append(1)
                if F[i, j] == H[i - 1, j] - gap_open:
                    state = 0
                i -= 1
            else:
                ops.append(2)
                if E[i, j] == H[i, j - 1] - gap_open:
                    state = 0
                j -= 1
        i0, j0 = i, j
        ops.reverse()
        runs, k = [], 0
        while k < len(ops):
            e = k
            while e < len(ops) and ops[e] == ops[k]:
                e += 1
            runs.append((e - k) << 2 | ops[k])
            k = e
    # the columns: (side, column) or None per side
    cols = [(x, None) for x in range(i0)] + [(None, y) for y in range(j0)]
    x, y = i0, j0
    for w in runs:
        ln, op = w >> 2, w & 3
        for _ in range(ln):
            if op == 0:
                cols.append((x, y)); x += 1; y += 1
            elif op == 1:
                cols.append((x, None)); x += 1
            else:
                cols.append((None, y)); y += 1
    assert (x, y) == (ie, je) and (i0 == 0 or j0 == 0) and (ie == Wa or je == Wb)
    cols += [(x, None) for x in range(ie, Wa)] + [(None, y) for y in range(je, Wb)]
    W = len(cols)
    cells = []
    for t in range(2):
        g = np.full((ma + mb, W), GAP, np.uint8)
        for c, (x, y) in enumerate(cols):
            if x is not None:
                g[:ma, c] = a[t][:, x]
            if y is not None:
                g[ma:, c] = b[t][:, y]
        cells.append(g)
    return {"score": sc, "is": i0, "js": j0, "ie": ie, "je": je, "runs": runs, "width": W, "cells": cells}


def check_merges(m, merges):
    """a merge list is a tree over the group: m - 1 merges, every child exists and is used once"""
    if len(merges) != m - 1:
        return False
    used = set()
    for k, (a, b) in enumerate(merges):
        if a == b or a >= m + k or b >= m + k or a in used or b in used:
            return False
        used |= {a, b}
    return True


def progressive_group(rows, merges, mats, gap_open, gap_ext):
    """rows: [(aa bytes, 3di bytes)] in file order.  Returns (width, [aa grid, 3di grid]) with the rows back in file order"""
    m = len(rows)
    assert check_merges(m, merges)
    nodes = [([np.frombuffer(bytes(r[0]), np.uint8).reshape(1, -1), np.frombuffer(bytes(r[1]), np.uint8).reshape(1, -1)], [k]) for k, r in enumerate(rows)]
    for a, b in merges:
        r = merge(nodes[a][0], nodes[b][0], mats, gap_open, gap_ext)
        nodes.append((r["cells"], nodes[a][1] + nodes[b][1]))
    cells, order = nodes[-1]
    back = np.argsort(np.array(order))
    return cells[0].shape[1], [c[back] for c in cells]


def progressive(grp_off, res_off, res, merges, S3, SA, gap_open, gap_ext):
    """the dict of unicore_amd.msa_progressive: {"width", "cells": [aa, 3di]} (flat, group after group); merges: per group a list of (a, b)"""
    go, ro = [int(x) for x in grp_off], [int(x) for x in res_off]
    mats = [np.asarray(SA).reshape(21, 21), np.asarray(S3).reshape(21, 21)]
    tr = [np.asarray(t, np.uint8) for t in res]
    width, out = [], [[], []]
    for g in range(len(go) - 1):
        rows = [(tr[0][ro[r]:ro[r + 1]], tr[1][ro[r]:ro[r + 1]]) for r in range(go[g], go[g + 1])]
        W, cells = progressive_group(rows, merges[g], mats, gap_open, gap_ext)
        width.append(W)
        for t in range(2):
            out[t].append(cells[t].reshape(-1))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return {"width": np.array(width, np.uint32), "cells": [cat(o) for o in out]}


def caterpillar(m):
    return [(0, 1)] + [(m + k - 1, k + 1) for k in range(1, m - 1)] if m > 1 else []


def balanced(m):
    """pairs level by level; an odd node out waits for the next level"""
    out, cur, nxt = [], list(range(m)), m
    while len(cur) > 1:
        new = []
        for k in range(0, len(cur) - 1, 2):
            out.append((cur[k], cur[k + 1])); new.append(nxt); nxt += 1
        if len(cur) & 1:
            new.append(cur[-1])
        cur = new
    return out


def tree_files(O, p, db_prefix, gene_files, threshold):
    """msa_ref.tree_files with the progressive MSA in the star MSA's place (the triangle is the one it computes for the centres).  Returns
    ({path: bytes}, info); info holds per gene also the self scores, D, the merge list and the root's width."""
    import bt_ref
    import msa_ref as R
    names, aa, di = R.read_db(db_prefix)
    id_of = {n: i for i, n in enumerate(names)}
    S3, SA = bt_ref.matrices(p)
    mats = [np.asarray(SA).reshape(21, 21), np.asarray(S3).reshape(21, 21)]
    files, info = R.tree_files(O, p, db_prefix, gene_files, threshold)
    kept = []
    for fn in sorted(f for f in gene_files if f.endswith(".txt")):
        gene = fn[:-4]
        rows = [l.split() for l in gene_files[fn].split(b"\n") if l != b""] if gene_files[fn] else []
        if not rows:
            continue
        m = len(rows)
        seq, species = [id_of[r[0]] for r in rows], [r[1] for r in rows]
        d = "fasta/%s/" % gene
        selfs = [self_score((np.frombuffer(aa[x], np.uint8), np.frombuffer(di[x], np.uint8)), mats) for x in seq]
        D, merges = guide(info[gene]["scores"], selfs)
        W, cells = progressive_group([(aa[x], di[x]) for x in seq], merges, mats, p.gap_open, p.gap_ext)
        cells = [c.reshape(-1) for c in cells]
        f = R.filter([0, m], [W], cells[0], threshold)
        fw = int(f["fwidth"][0])
        fasta = lambda c, w: b"".join(b">" + species[i] + b"\n" + c[i * w:(i + 1) * w].tobytes() + b"\n" for i in range(m))
        files[d + gene + ".fa"] = fasta(cells[0], W)
        files[d + gene + "_3di.fa"] = fasta(cells[1], W)
        files[d + gene + ".fa.filtered"] = fasta(f["fcells"], fw)
        info[gene].update(self=selfs, D=D, merges=merges, width=W)
        if fw:
            kept.append((gene, species, f["fcells"].reshape(m, fw), fw))
    order, at, parts = [], 0, []
    for _, species, _, _ in kept:
        for s in species:
            if s not in order:
                order.append(s)
    seqs = {s: [] for s in order}
    for gene, species, grid, fw in kept:
        for s in order:
            seqs[s].append(grid[species.index(s)].tobytes() if s in species else b"-" * fw)
        parts.append(b"JTT+F+I+G, %s=%d-%d\n" % (gene.encode(), at + 1, at + fw))
        at += fw
    files["combined.fasta"] = b"".join(b">" + s + b"\n" + b"".join(seqs[s]) + b"\n" for s in order)
    files["combined.fasta.partitions"] = b"".join(parts)
    return files, info
