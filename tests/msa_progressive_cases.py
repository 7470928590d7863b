"""The shared case list of rule UC-T/G (`unicore tree -a progressive`): keyword sets of unicore_amd.msa_merge, msa_progressive and msa_guide, for the CPU
tests (twin against reference) and the GPU tests (kernels against twin against reference).  Everything is seeded; nothing here calls product code."""
import numpy as np

import msa_progressive_ref as G

LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYX", np.uint8)
GAP = G.GAP
WIDTHS = (1, 63, 64, 65, 129)
ROWS = ((1, 1), (1, 2), (3, 5), (40, 60))
TREE_ROWS = (1, 2, 3, 4, 9, 33)


def matrices(rng, lo=-9, hi=12):
    """SA, S3: random, asymmetric, a heavier diagonal"""
    out = []
    for _ in range(2):
        S = rng.integers(lo, hi, (21, 21))
        S[np.arange(21), np.arange(21)] += 6
        out.append(S.astype(np.int8))
    return out


def node(rng, m, W, alphabet=21, gap_rate=0.3):
    """[aa grid, 3di grid] of m x W: the tracks agree on gaps, every column holds a residue"""
    aa, di = LETTERS[rng.integers(0, alphabet, (m, W))], LETTERS[rng.integers(0, alphabet, (m, W))]
    gap = rng.random((m, W)) < (gap_rate if m > 1 else 0.0)
    if W:
        gap[rng.integers(0, m, W), np.arange(W)] = False
    aa, di = aa.copy(), di.copy()
    aa[gap] = GAP; di[gap] = GAP
    return [aa, di]


def merge_kw(tasks, S, gap_open, gap_ext):
    """tasks: [(a, b)] of nodes"""
    cat = lambda parts: np.concatenate([p.reshape(-1) for p in parts]) if parts else np.zeros(0, np.uint8)
    return dict(ma=[a[0].shape[0] for a, _ in tasks], mb=[b[0].shape[0] for _, b in tasks], Wa=[a[0].shape[1] for a, _ in tasks], Wb=[b[0].shape[1] for _, b in tasks],
                a=[cat([a[t] for a, _ in tasks]) for t in range(2)], b=[cat([b[t] for _, b in tasks]) for t in range(2)], SA=S[0], S3=S[1], gap_open=gap_open, gap_ext=gap_ext)


def tasks_of(kw):
    """the (a, b) nodes of a keyword set"""
    out, oa, ob = [], 0, 0
    for ma, mb, Wa, Wb in zip(kw["ma"], kw["mb"], kw["Wa"], kw["Wb"]):
        out.append(([kw["a"][t][oa:oa + ma * Wa].reshape(ma, Wa) for t in range(2)], [kw["b"][t][ob:ob + mb * Wb].reshape(mb, Wb) for t in range(2)]))
        oa += ma * Wa; ob += mb * Wb
    return out


def related(rng, m, L, sub=0.25, indel=0.08):
    """m rows [(aa, 3di)] mutated from one ancestor of L residues; lengths differ"""
    anc = (rng.integers(0, 20, L), rng.integers(0, 20, L))
    rows = []
    for _ in range(m):
        keep = rng.random(L) >= indel
        x, y = anc[0][keep].copy(), anc[1][keep].copy()
        ch = rng.random(len(x)) < sub
        x[ch] = rng.integers(0, 20, int(ch.sum())); y[ch] = rng.integers(0, 20, int(ch.sum()))
        lo, hi = int(rng.integers(0, 4)), len(x) - int(rng.integers(0, 4))
        rows.append((LETTERS[x[lo:hi]], LETTERS[y[lo:hi]]))
    return rows


def merge_cases():
    """{name: keyword set of msa_merge}"""
    out = {}
    rng = np.random.default_rng(20261021)
    S = matrices(rng)
    out["widths"] = merge_kw([(node(rng, 2, Wa), node(rng, 3, Wb)) for Wa in WIDTHS for Wb in WIDTHS], S, 11, 1)
    low = matrices(rng, -12, 9)      # a mean below 0: sums of many rows are negative too, so the floor division rounds a negative quotient
    for ma, mb in ROWS:
        out["rows_%d_%d" % (ma, mb)] = merge_kw([(node(rng, ma, 37), node(rng, mb, 45))], low, 9, 2)
    out["many"] = merge_kw([(node(rng, int(rng.integers(1, 4)), int(rng.integers(1, 24))), node(rng, int(rng.integers(1, 4)), int(rng.integers(1, 24)))) for _ in range(300)], S, 7, 1)
    # +-48 on mirrored cells: swapping the sides must change the answer
    asym = [np.zeros((21, 21), np.int8) for _ in range(2)]
    for S_ in asym:
        for x in range(21):
            for y in range(21):
                S_[x, y] = 48 if x < y else -48 if x > y else 5
    a, b = node(rng, 2, 40, alphabet=6), node(rng, 2, 33, alphabet=6)
    out["asymmetric"] = merge_kw([(a, b)], asym, 20, 3)
    out["asymmetric_swapped"] = merge_kw([(b, a)], asym, 20, 3)
    # ties: few letters, a matrix of -1 .. 1, gaps that cost nothing
    tie = [rng.integers(-1, 2, (21, 21)).astype(np.int8) for _ in range(2)]
    out["ties"] = merge_kw([(node(rng, 1, 30, alphabet=3), node(rng, 2, 41, alphabet=3)) for _ in range(6)], tie, 0, 0)
    out["open_eq_ext"] = merge_kw([(node(rng, 2, 70), node(rng, 2, 50)), (node(rng, 1, 20), node(rng, 3, 66))], S, 3, 3)
    neg = [np.full((21, 21), -5, np.int8) for _ in range(2)]
    out["all_negative"] = merge_kw([(node(rng, 2, 17), node(rng, 1, 70))], neg, 4, 1)
    # overhangs on both ends: a = its own prefix + a core, b = the core + its own suffix
    ident = [(np.eye(21) * 12 - 4).astype(np.int8) for _ in range(2)]
    core, pre, suf = node(rng, 1, 60), node(rng, 1, 25), node(rng, 1, 31)
    out["overhangs"] = merge_kw([([np.concatenate([pre[t], core[t]], axis=1) for t in range(2)], [np.concatenate([core[t], suf[t]], axis=1) for t in range(2)])], ident, 10, 1)
    # every letter the checks accept: lower case, and B J O U X Z, which code as 20
    every = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", np.uint8)
    def spelled(nd):
        return [np.where(g == GAP, GAP, every[rng.integers(0, len(every), g.shape)]).astype(np.uint8) for g in nd]
    out["letters"] = merge_kw([(spelled(node(rng, 3, 70)), spelled(node(rng, 2, 66))), (spelled(node(rng, 1, 30)), spelled(node(rng, 4, 9)))], S, 8, 1)
    out["width_0"] = merge_kw([(node(rng, 1, 0), node(rng, 2, 7)), (node(rng, 3, 9), node(rng, 1, 0)), (node(rng, 1, 0), node(rng, 1, 0)), (node(rng, 2, 5), node(rng, 2, 6))], S, 11, 1)
    return out


def progressive_cases():
    """{name: keyword set of msa_progressive}: forced caterpillar and balanced merge lists"""
    out = {}
    rng = np.random.default_rng(42)
    S = [(np.eye(21) * 10 - 3 + rng.integers(-1, 2, (21, 21))).astype(np.int8) for _ in range(2)]
    for m in TREE_ROWS:
        rows = related(rng, m, 90 if m < 33 else 40)
        if m >= 4:
            rows[2] = (np.zeros(0, np.uint8), np.zeros(0, np.uint8))      # a row without a residue
        res_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.uint64)
        res = [np.concatenate([r[t] for r in rows]) for t in range(2)]
        for shape, ml in (("caterpillar", G.caterpillar(m)), ("balanced", G.balanced(m))):
            out["%s_%d" % (shape, m)] = dict(grp_off=[0, m], res_off=res_off, res=res, merges=[np.array(ml, np.uint32).reshape(-1, 2)], SA=S[0], S3=S[1], gap_open=10, gap_ext=1)
    # several groups in one call: the levels of all groups run together
    groups = [related(rng, m, 50) for m in (3, 1, 5, 2)]
    rows = [r for g in groups for r in g]
    out["several_groups"] = dict(grp_off=np.concatenate([[0], np.cumsum([len(g) for g in groups])]), res_off=np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.uint64),
                                 res=[np.concatenate([r[t] for r in rows]) for t in range(2)],
                                 merges=[np.array(G.balanced(len(g)) if k & 1 else G.caterpillar(len(g)), np.uint32).reshape(-1, 2) for k, g in enumerate(groups)],
                                 SA=S[0], S3=S[1], gap_open=10, gap_ext=1)
    return out


def leaf_sum_case():
    """(m, L, keyword set of msa_progressive without its merge list): 1000 rows of 100 residues from one ancestor, substitutions only.  The residues below the
    two sides of a balanced tree's top merge multiply to more than 2^31, while every node stays about 100 columns wide"""
    rng = np.random.default_rng(31)
    m, L = 1000, 100
    anc = rng.integers(0, 20, (2, L))
    res = []
    for t in range(2):
        rows = np.tile(anc[t], (m, 1))
        ch = rng.random((m, L)) < 0.2
        rows[ch] = rng.integers(0, 20, int(ch.sum()))
        res.append(LETTERS[rows].reshape(-1))
    S = (np.eye(21) * 10 - 3).astype(np.int8)
    return m, L, dict(grp_off=[0, m], res_off=np.arange(m + 1) * L, res=res, SA=S, S3=S, gap_open=10, gap_ext=1)


def guide_cases(big=False):
    """{name: (grp_off, scores, self_scores)}; big adds a group above the device join's threshold"""
    rng = np.random.default_rng(7)
    out = {}
    ms = (1, 2, 3, 5, 24) + ((260,) if big else ())
    selfs = np.concatenate([rng.integers(50, 900, m) for m in ms]).astype(np.int64)
    selfs[3] = 0                      # den <= 0: D = 1
    tri = np.concatenate([rng.integers(-20, 700, m * (m - 1) // 2) for m in ms]).astype(np.int32)      # scores above the self score clamp at 0
    out["mixed"] = (np.concatenate([[0], np.cumsum(ms)]).astype(np.uint64), tri, selfs)
    return out
