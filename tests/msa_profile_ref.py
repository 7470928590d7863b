"""Test-side restatement of rule UC-T/P (`unicore tree -a profile`): one profile refinement round of a group's MSA in plain
Python over bt_ref.dp: the leave-one-out profile with floor division, the E5 recurrence on columns x residues, the end cell (largest score, smallest
residue, smallest column), one walk on the full matrix with E6's preferences, the layout UC-T/L with a virtual centre and the drop of the columns
without an amino acid.  Track 0 is the amino acids, track 1 the 3Di letters.  No product code is involved."""
import numpy as np

import bt_ref

GAP = ord("-")
LET = "ACDEFGHIKLMNPQRSTVWY"
CODE = np.full(256, 20, np.uint8)
for _k, _c in enumerate(LET):
    CODE[ord(_c)] = CODE[ord(_c.lower())] = _k


def profile(grid, S, r):
    """P_r [W][21] of one track: grid [m][W] bytes, S [21][21] = [column letter][row letter]; Python's // is the floor"""
    m, W = grid.shape
    P = np.zeros((W, 21), np.int64)
    for c in range(W):
        for i in range(m):
            if i != r and grid[i, c] != GAP:
                P[c] += S[CODE[grid[i, c]]]
    return P // (m - 1)


def align_row(grids, res, mats, r, gap_open, gap_ext):
    """(aligned, score, qs, ts, qe, te, runs) of row r: grids / res / mats are per track [aa, 3di]"""
    m, W = grids[0].shape
    L = len(res[0])
    if m < 2 or W == 0 or L == 0:
        return 0, 0, 0, 0, 0, 0, []
    S = sum(profile(grids[t], np.asarray(mats[t], np.int64), r)[:, CODE[res[t]]] for t in range(2)).astype(np.int32)
    H, E, F = bt_ref.dp(S, gap_open, gap_ext)
    score = int(H.max())
    if score <= 0:
        return 0, score, 0, 0, 0, 0, []
    te = min(j for j in range(1, L + 1) if (H[:, j] == score).any())
    qe = min(i for i in range(1, W + 1) if H[i, te] == score)
    i, j, state, ops = qe, te, 0, []
    while i > 0 and j > 0:
        if state == 0:
            h = H[i, j]
            if h == 0:
                break
            if h == H[i - 1, j - 1] + S[i - 1, j - 1]:
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
    ops.reverse()
    runs, k = [], 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        runs.append((e - k) << 2 | ops[k])
        k = e
    return 1, score, i, j, qe - 1, te - 1, runs      # i, j: one before the first cell in 1-based = the first cell in 0-based


def cell_scores(grids, res, mats, r):
    """s_r [W][L] of row r, for the path checks"""
    return sum(profile(grids[t], np.asarray(mats[t], np.int64), r)[:, CODE[res[t]]] for t in range(2))


def _split(grp_off, width, cells):
    go, out, o = [int(x) for x in grp_off], [], 0
    for g in range(len(go) - 1):
        m, W = go[g + 1] - go[g], int(width[g])
        out.append([np.asarray(c, np.uint8)[o:o + m * W].reshape(m, W) for c in cells])
        o += m * W
    return go, out


def align(grp_off, width, cells, res_off, res, S3, SA, gap_open, gap_ext):
    """the dict of unicore_amd.msa_profile_align"""
    go, grids = _split(grp_off, width, cells)
    ro = [int(x) for x in res_off]
    mats = [np.asarray(SA).reshape(21, 21), np.asarray(S3).reshape(21, 21)]
    keys = ("aligned", "score", "qs", "ts", "qe", "te")
    out, run_off, runs = {k: [] for k in keys}, [0], []
    for g in range(len(go) - 1):
        for r in range(go[g], go[g + 1]):
            row = [np.asarray(t, np.uint8)[ro[r]:ro[r + 1]] for t in res]
            a = align_row(grids[g], row, mats, r - go[g], gap_open, gap_ext)
            for k, v in zip(keys, a[:6]):
                out[k].append(v)
            runs.extend(a[6]); run_off.append(len(runs))
    res_ = {k: np.array(v, np.uint8 if k == "aligned" else np.int32) for k, v in out.items()}
    res_["run_off"], res_["runs"] = np.array(run_off, np.uint64), np.array(runs, np.uint32)
    return res_


def layout(grp_off, width, cells, res_off, res, aligned, qs, ts, run_off, runs):
    """the dict of unicore_amd.msa_profile_layout: {"width", "cells": [aa, 3di]}"""
    go, grids = _split(grp_off, width, cells)
    ro, uo = [int(x) for x in res_off], [int(x) for x in run_off]
    tracks = [np.asarray(t, np.uint8) for t in res]
    new_w, out = [], [[], []]
    for g in range(len(go) - 1):
        b, m, W = go[g], go[g + 1] - go[g], int(width[g])
        if m == 1:
            new_w.append(W)
            for t in range(2):
                out[t].append(grids[g][t].reshape(-1))
            continue
        ins = [0] * (W + 1)
        for r in range(b, b + m):
            if aligned[r]:
                s = int(qs[r])
                for w in runs[uo[r]:uo[r + 1]]:
                    ln, op = int(w) >> 2, int(w) & 3
                    if op == 2:
                        ins[s] = max(ins[s], ln)
                    else:
                        s += ln
        cx = [s + sum(ins[:s + 1]) for s in range(W + 1)]
        W2 = cx[W]
        new = [np.full((m, W2), GAP, np.uint8) for _ in range(2)]
        for k in range(2):
            for r in range(b, b + m):
                if not aligned[r]:
                    continue
                x = tracks[k][ro[r]:ro[r + 1]]
                s, t = int(qs[r]), int(ts[r])
                for w in runs[uo[r]:uo[r + 1]]:
                    ln, op = int(w) >> 2, int(w) & 3
                    if op == 0:
                        for l in range(ln):
                            new[k][r - b, cx[s + l]] = x[t + l]
                        s += ln; t += ln
                    elif op == 1:
                        s += ln
                    else:
                        first = cx[s] - ins[s]
                        new[k][r - b, first:first + ln] = x[t:t + ln]
                        t += ln
        keep = (new[0] != GAP).any(axis=0) if W2 else np.zeros(0, bool)
        new_w.append(int(keep.sum()))
        for k in range(2):
            out[k].append(new[k][:, keep].reshape(-1))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return {"width": np.array(new_w, np.uint32), "cells": [cat(o) for o in out]}


def refine(grp_off, width, cells, res_off, res, S3, SA, gap_open, gap_ext, rounds):
    """`rounds` rounds; returns (width, cells, [the align dict of every round])"""
    log = []
    for _ in range(rounds):
        a = align(grp_off, width, cells, res_off, res, S3, SA, gap_open, gap_ext)
        l = layout(grp_off, width, cells, res_off, res, a["aligned"], a["qs"], a["ts"], a["run_off"], a["runs"])
        width, cells = l["width"], l["cells"]
        log.append(a)
    return width, cells, log


def sum_of_pairs(grids, mats, gap_open, gap_ext):
    """the sum-of-pairs score of one group's MSA (tracks [aa, 3di]) under the matrices and affine gaps; columns where both rows hold a gap are skipped"""
    m, W = grids[0].shape
    tot = 0
    for a in range(m):
        for b in range(a + 1, m):
            state = 0
            for c in range(W):
                ga, gb = grids[0][a, c] == GAP, grids[0][b, c] == GAP
                if ga and gb:
                    continue
                if not ga and not gb:
                    tot += sum(int(mats[t][CODE[grids[t][a, c]], CODE[grids[t][b, c]]]) for t in range(2))
                    state = 0
                else:
                    s = 1 if ga else 2
                    tot -= gap_ext if state == s else gap_open
                    state = s
    return tot


def tree_files(O, p, db_prefix, gene_files, threshold, rounds):
    """msa_ref.tree_files with `rounds` rounds of UC-T/P between the star MSA and the filter.  Returns ({path: bytes}, info)."""
    import msa_ref as R
    names, aa, di = R.read_db(db_prefix)
    id_of = {n: i for i, n in enumerate(names)}
    S3, SA = bt_ref.matrices(p)
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
        rd = lambda path: [np.frombuffer(l, np.uint8) for l in files[path].split(b"\n")[1::2]]
        g_aa, g_3di = np.array(rd(d + gene + ".fa")), np.array(rd(d + gene + "_3di.fa"))
        W = g_aa.shape[1]
        res_off = np.concatenate([[0], np.cumsum([len(aa[x]) for x in seq])])
        res = [np.frombuffer(b"".join(aa[x] for x in seq), np.uint8), np.frombuffer(b"".join(di[x] for x in seq), np.uint8)]
        width, cells, log = refine([0, m], [W], [g_aa.reshape(-1), g_3di.reshape(-1)], res_off, res, S3, SA, p.gap_open, p.gap_ext, rounds)
        W = int(width[0])
        import msa_ref
        f = msa_ref.filter([0, m], width, cells[0], threshold)
        fw = int(f["fwidth"][0])
        fasta = lambda c, w: b"".join(b">" + species[i] + b"\n" + c[i * w:(i + 1) * w].tobytes() + b"\n" for i in range(m))
        files[d + gene + ".fa"] = fasta(cells[0], W)
        files[d + gene + "_3di.fa"] = fasta(cells[1], W)
        files[d + gene + ".fa.filtered"] = fasta(f["fcells"], fw)
        info[gene]["refine"] = [{k: v.tolist() for k, v in a.items()} for a in log]
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
