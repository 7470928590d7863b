"""Test-side restatement of rule UC-T (`unicore tree --no-inference`): centre (UC-T/C), layout (UC-T/L), rows, filter (UC-T/F) and the
concatenation, in plain Python on the arrays the entry points take.  The alignments come from the oracle's `sw` and from bt_ref.box_of /
bt_ref.traceback, the reference the backtrace tests hold the device to.  No product code is involved.

The fixed options of the centre -> member pass (-e 1e30 -c 0 --cov-mode 0 --min-seq-id 0 --rev-correction 0) leave one gate: a pair is accepted
iff its forward score is positive (oracle/uc_oracle.c, uco_align_pair: min_score = 1, corrected = score, no coverage or identity threshold)."""
import hashlib
import os

import numpy as np

import bt_ref

OP = {"M": 0, "I": 1, "D": 2}
GAP = ord("-")
FIXED_OPTS = "-e 1e30 -c 0 --cov-mode 0 --min-seq-id 0 --rev-correction 0 --max-seqs 65535"


# ---- UC-T/C ---------------------------------------------------------------------------------------------------------------------------------
def center(grp_off, scores):
    go = [int(x) for x in grp_off]
    sc = [int(x) for x in scores]
    out, k = [], 0
    for g in range(len(go) - 1):
        m = go[g + 1] - go[g]
        s = [0] * m
        for i in range(m):
            for j in range(i + 1, m):
                s[i] += sc[k]; s[j] += sc[k]
                k += 1
        out.append(max(range(m), key=lambda i: (s[i], -i)))
    return np.array(out, np.uint32)


# ---- UC-T/L and the rows ------------------------------------------------------------------------------------------------------------------
def _events(qs, ts, runs):
    """(matches [(centre position, row position)], inserts {slot: (row position, length)}) of one aligned row"""
    s, t, match, ins = int(qs), int(ts), [], {}
    for w in runs:
        ln, op = int(w) >> 2, int(w) & 3
        if op == 0:
            match.extend((s + l, t + l) for l in range(ln))
            s += ln; t += ln
        elif op == 1:
            s += ln
        else:
            assert s not in ins
            ins[s] = (t, ln)
            t += ln
    return match, ins


def star(grp_off, centre, res_off, res, qs, ts, run_off, runs, aligned):
    """the dict of unicore_amd.msa_star"""
    tracks = [np.asarray(t, np.uint8) for t in (res if isinstance(res, (list, tuple)) else [res])]
    go, ro, uo = [int(x) for x in grp_off], [int(x) for x in res_off], [int(x) for x in run_off]
    width, col, cnt, cells = [], [], [], [[] for _ in tracks]
    for g in range(len(go) - 1):
        b, m = go[g], go[g + 1] - go[g]
        c = b + int(centre[g])
        Lc = ro[c + 1] - ro[c]
        ev = {}
        for r in range(b, b + m):
            if r != c and aligned[r]:
                ev[r] = _events(qs[r], ts[r], runs[uo[r]:uo[r + 1]])
        ins = [max([e[1][s][1] for e in ev.values() if s in e[1]] or [0]) for s in range(Lc + 1)]
        cx = [s + sum(ins[:s + 1]) for s in range(Lc + 1)]       # cx[Lc] is the width
        W = cx[Lc]
        assert W == Lc + sum(ins)
        width.append(W); col.extend(cx[:Lc])
        grid = [np.full((m, W), GAP, np.uint8) for _ in tracks]
        for k, tr in enumerate(tracks):
            for r in range(b, b + m):
                x = tr[ro[r]:ro[r + 1]]
                if r == c:
                    for p in range(Lc):
                        grid[k][r - b, cx[p]] = x[p]
                elif r in ev:
                    for p, q in ev[r][0]:
                        grid[k][r - b, cx[p]] = x[q]
                    for s, (q, ln) in ev[r][1].items():
                        first = cx[s] - ins[s]
                        grid[k][r - b, first:first + ln] = x[q:q + ln]
            cells[k].append(grid[k].reshape(-1))
        cnt.extend((grid[0] != GAP).sum(axis=0).tolist())
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return {"width": np.array(width, np.uint32), "col": np.array(col, np.uint32), "cnt": np.array(cnt, np.uint32), "cells": [cat(c) for c in cells]}


# ---- UC-T/F -----------------------------------------------------------------------------------------------------------------------------------
def filter(grp_off, width, cells, threshold):
    """the dict of unicore_amd.msa_filter"""
    go, cells = [int(x) for x in grp_off], np.asarray(cells, np.uint8)
    keep, fwidth, fcells, o = [], [], [], 0
    for g in range(len(go) - 1):
        m, W = go[g + 1] - go[g], int(width[g])
        grid = cells[o:o + m * W].reshape(m, W)
        o += m * W
        k = np.array([int((grid[:, c] != GAP).sum()) * 100 >= threshold * m for c in range(W)], bool)
        keep.extend(k.astype(np.uint8).tolist()); fwidth.append(int(k.sum()))
        fcells.append(grid[:, k].reshape(-1))
    return {"keep": np.array(keep, np.uint8), "fwidth": np.array(fwidth, np.uint32),
            "fcells": np.concatenate(fcells) if fcells else np.zeros(0, np.uint8)}


# ---- alignments from the oracle ------------------------------------------------------------------------------------------------------------------
def pair_scores(O, p, s3, sa):
    """the packed upper triangle of one group: forward gapped score, row i as query"""
    return [O.sw(s3[i], sa[i], s3[j], sa[j], p)[0] for i in range(len(s3)) for j in range(i + 1, len(s3))]


def align_to_centre(O, p, s3, sa, c):
    """per row (aligned, qs, ts, run words) with row c as query; the centre's own entry is (1, 0, 0, [])"""
    S3, SA = bt_ref.matrices(p)
    out = []
    for r in range(len(s3)):
        if r == c:
            out.append((1, 0, 0, []))
            continue
        b = bt_ref.box_of(O, p, s3[c], sa[c], s3[r], sa[r])
        if b is None:
            out.append((0, 0, 0, []))
            continue
        s, qs, qe, ts, te = b
        tb = bt_ref.traceback(s3[c][qs:qe + 1], sa[c][qs:qe + 1], s3[r][ts:te + 1], sa[r][ts:te + 1], S3, SA, p.gap_open, p.gap_ext)
        assert tb[4] == s
        out.append((1, qs, ts, [n << 2 | OP[op] for n, op in bt_ref.parse(tb[3])]))
    return out


# ---- the file level ------------------------------------------------------------------------------------------------------------------------------
def read_db(prefix):
    """names (first token of the header), amino-acid and 3Di letters as stored, in key order"""
    def entries(path):
        data = open(path, "rb").read()
        idx = sorted(tuple(int(x) for x in l.split()) for l in open(path + ".index"))
        return [data[o:o + n - 2] for _, o, n in idx]
    return [h.split()[0] if h.split() else b"" for h in entries(prefix + "_h")], entries(prefix), entries(prefix + "_ss")


def tree_files(O, p, db_prefix, gene_files, threshold):
    """gene_files: {file name: bytes} of a profile directory.  Returns ({path relative to the output directory: bytes}, info) where info holds,
    per gene, its centre and its packed triangle."""
    names, aa, di = read_db(db_prefix)
    id_of = {n: i for i, n in enumerate(names)}
    files, info, kept = {}, {}, []
    for fn in sorted(f for f in gene_files if f.endswith(".txt")):
        gene = fn[:-4]
        rows = [l.split() for l in gene_files[fn].split(b"\n") if l != b""] if gene_files[fn] else []
        assert all(len(r) == 2 for r in rows)
        seq, species = [id_of[r[0]] for r in rows], [r[1] for r in rows]
        d = "fasta/%s/" % gene
        files[d + "aa.fasta"] = b"".join(b">" + s + b"\n" + aa[x] + b"\n" for s, x in zip(species, seq))
        files[d + "3di.fasta"] = b"".join(b">" + s + b"\n" + di[x] + b"\n" for s, x in zip(species, seq))
        if not rows:
            continue
        m = len(rows)
        s3, sa = [O.encode(di[x]) for x in seq], [O.encode(aa[x]) for x in seq]
        tri = pair_scores(O, p, s3, sa)
        c = int(center([0, m], tri)[0])
        al = align_to_centre(O, p, s3, sa, c)
        res_off = np.concatenate([[0], np.cumsum([len(aa[x]) for x in seq])])
        run_off = np.concatenate([[0], np.cumsum([len(a[3]) for a in al])])
        r = star([0, m], [c], res_off, [np.frombuffer(b"".join(aa[x] for x in seq), np.uint8), np.frombuffer(b"".join(di[x] for x in seq), np.uint8)],
                 [a[1] for a in al], [a[2] for a in al], run_off, [w for a in al for w in a[3]], [a[0] for a in al])
        W = int(r["width"][0])
        f = filter([0, m], r["width"], r["cells"][0], threshold)
        fw = int(f["fwidth"][0])
        fasta = lambda cells, w: b"".join(b">" + species[i] + b"\n" + cells[i * w:(i + 1) * w].tobytes() + b"\n" for i in range(m))
        files[d + gene + ".fa"] = fasta(r["cells"][0], W)
        files[d + gene + "_3di.fa"] = fasta(r["cells"][1], W)
        files[d + gene + ".fa.filtered"] = fasta(f["fcells"], fw)
        info[gene] = {"centre": c, "scores": tri, "unaligned": sum(1 for a in al if not a[0])}
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
    files["tree.chk"] = b"0"
    return files, info


def digest(files):
    """what the committed fixture keeps: the two concatenation files in full, a sha256 per gene file"""
    return {"combined.fasta": files["combined.fasta"].decode("ascii"), "combined.fasta.partitions": files["combined.fasta.partitions"].decode("ascii"),
            "tree.chk": files["tree.chk"].decode("ascii"),
            "sha256": {k: hashlib.sha256(v).hexdigest() for k, v in sorted(files.items()) if k.startswith("fasta/")}}


def read_tree(out_dir):
    """{relative path: bytes} of an output directory"""
    got = {}
    for root, _, fs in os.walk(out_dir):
        for f in fs:
            p = os.path.join(root, f)
            got[os.path.relpath(p, out_dir)] = open(p, "rb").read()
    return got
