"""Pairs that sit exactly on the thresholds of the accept gates of stage E5 / E6 (length gate UC-1/L, E-value gate, coverage gate, identity
gate), built in code from seeds so that their alignment is known in advance, with the record each gate must produce.

Construction.  A core of k random residues (both tracks) is embedded in runs of one flank letter: query = fq^x . core . fq^(Lq-k-x), target =
ft^y . core' . ft^(Lt-k-y), where (fq, ft) is the letter pair with the most negative combined score S3 + SA of the matrices in use (-14 with the
stand-in 3Di matrix).  The optimal local alignment is the core against itself: qstart = x, qend = x + k - 1, tstart = y, tend = y + k - 1.
  span cases      core' = core: spans k / Lq and k / Lt.  One trio per grid point (k, L): A = flanked by fq (L residues), B = the bare core (k),
                  C = flanked by ft (L); the pairs (A, B), (B, A), (A, C), (C, A) put the boundary on qcov alone, tcov alone and both, and every
                  pair is in the lists in both directions (mutual hits).
  identity cases  m AA letters of core' differ at interior positions, the 3Di track is left alone: every column still scores >= 0 and the end
                  columns > 0 (asserted on the matrices), so aln_len = k and idents = k - m.  Gapped variant: 3 interior residues of the
                  target's core are deleted as well, substitutions stay 3 positions away: aln_len = k, idents = k - 3 - m, one gap.
Nothing of this is assumed: a block of sequences is generated from (family, k, L, attempt) and handed out only once the scalar oracle gives the
intended record for every pair of it; the attempt counter moves on otherwise (tests/test_gate_cases.py checks every shipped pair again and pins
the counts).  The E-value gate is taken out of the span and identity cases by `-e 1e30` (threshold 1 for every query); the eval family sets it
per query with --min-score-table.

The closed-form expectation (expected()) is the intended integers pushed through the spec's rule in numpy.float32 -
np.float32(a) / np.float32(b) >= np.float32(thr) - and is the reference both the oracle and the engine are compared with.
"""
import functools

import numpy as np

import util

FIELDS = ("score", "score_rev", "corrected", "qstart", "qend", "tstart", "tend", "aln_len", "idents", "pass_evalue", "accepted", "gap_opens")
E1 = "-e 1e30"                  # Karlin-Altschul threshold 1 for every query length
COV_THRESHOLDS = (0.8, 0.6, 0.3, 0.1, 0.85, 0.5, 1.0)       # the float of the first five differs from the decimal; 0.5 and 1.0 are exact
SID_THRESHOLDS = (0.9, 0.6, 0.3, 0.2, 1.0)
LEN_THRESHOLDS = (0.8, 0.5)
GRID_L = tuple(range(5, 201, 5))
EXTRA_L_HALF = (82, 94, 110, 122)                           # 0.5 only: lengths L with float(L / 2) * (1 / float(L)) < 0.5
SID_K = tuple(sorted(set(range(10, 201, 10)) | {7, 13, 33, 77, 150}))
GAP = 3                         # residues deleted from the target's core in the gapped identity cases
GAP_MIN_K = 13                  # the smallest core that leaves three untouched columns on either side of the deletion
PK_LIMIT = 0x7C00 - 256         # scores from here on leave the packed kernels' range and are re-run in int32
SYS_ROWS = 2048                 # queries of more residues take the long-query kernel


def rnd(x):
    """round half up: the grid's centre"""
    return int(np.floor(x + 0.5))


def f32_ge(a, b, thr):
    """the spec's rule: float division, float comparison"""
    return bool(np.float32(a) / np.float32(b) >= np.float32(thr))


def double_ge(a, b, thr):
    """near miss (i): the quotient formed in double and compared with (double)(float)thr"""
    return float(a) / float(b) >= float(np.float32(thr))


def recip_ge(a, b, thr):
    """near miss (ii): a * (1 / b) in float"""
    return bool(np.float32(a) * (np.float32(1) / np.float32(b)) >= np.float32(thr))


@functools.lru_cache(maxsize=None)
def _O():
    from oracle import oracle_py
    return oracle_py


@functools.lru_cache(maxsize=None)
def base_params():
    """threshold 1, no coverage gate, traceback statistics for every pair: what the landing check runs under"""
    p = util.oracle_params(_O(), "-c 0 " + E1)
    p.want_tb = 1
    return p


@functools.lru_cache(maxsize=None)
def matrices():
    p = base_params()
    return (np.array(p.S3[:], np.int64).reshape(21, 21)[:20, :20].copy(), np.array(p.SA[:], np.int64).reshape(21, 21)[:20, :20].copy())


@functools.lru_cache(maxsize=None)
def letters():
    """fq, ft: the flank residues (3Di, AA) of query and target, worst: their combined score; best: the residue with the highest
    self-score, second: the same 3Di letter with the second-best AA letter"""
    S3, SA = matrices()
    i3, ia = np.unravel_index(np.argmin(S3), S3.shape), np.unravel_index(np.argmin(SA), SA.shape)
    b3, ba = int(np.argmax(np.diag(S3))), np.argsort(-np.diag(SA), kind="stable")
    return dict(fq=(int(i3[0]), int(ia[0])), ft=(int(i3[1]), int(ia[1])), worst=int(S3[i3] + SA[ia]),
                best=(b3, int(ba[0])), second=(b3, int(ba[1])), best_score=int(S3[b3, b3] + SA[ba[0], ba[0]]))


def _rnd(rng, n):
    return rng.integers(0, 20, n, dtype=np.uint8), rng.integers(0, 20, n, dtype=np.uint8)


def _rep(letter, n):
    return np.full(n, letter[0], np.uint8), np.full(n, letter[1], np.uint8)


def _cat(*parts):
    return np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts])


def _flanked(core, letter, x, total):
    return _cat(_rep(letter, x), core, _rep(letter, total - len(core[0]) - x))


def _columns(a, b):
    S3, SA = matrices()
    return S3[a[0], b[0]] + SA[a[1], b[1]]


def _want(score, qs, ts, k, lt_span, idents, gaps):
    return dict(score=int(score), qstart=qs, qend=qs + k - 1, tstart=ts, tend=ts + lt_span - 1, aln_len=k, idents=idents, gap_opens=gaps)


def _swapped(w):
    return dict(w, qstart=w["tstart"], qend=w["tend"], tstart=w["qstart"], tend=w["qend"])


# ---- blocks: a few sequences and the pairs among them, each pair (q, t, layout, want) ----------------------------------------------------
def _span_block(rng, k, L, core=None):
    core = _rnd(rng, k) if core is None else core
    x, y = int(rng.integers(0, L - k + 1)), int(rng.integers(0, L - k + 1))
    ln = letters()
    seqs = [_flanked(core, ln["fq"], x, L), core, _flanked(core, ln["ft"], y, L)]
    s = _columns(core, core).sum()
    ab, ac = _want(s, x, 0, k, k, k, 0), _want(s, x, y, k, k, k, 0)
    return seqs, [(0, 1, "(Lq,Lt)=(L,k)", ab), (1, 0, "(Lq,Lt)=(k,L)", _swapped(ab)), (0, 2, "(Lq,Lt)=(L,L)", ac), (2, 0, "(Lq,Lt)=(L,L) swapped", _swapped(ac))]


def sid_sites(k, gapped):
    """(positions of the core that may be substituted, first deleted position): interior, and 3 away from the deletion"""
    p = k // 2 - 1
    return [i for i in range(1, k - 1) if not gapped or i <= p - 3 or i >= p + GAP + 2], p


def sid_variants(s, k):
    """(m, gapped) of the identity cases of core length k at threshold s: idents = round(s k) + {-1, 0, 1}, moved into the range the
    construction reaches (ungapped: 2 .. k identities, gapped: k - 3 - sites .. k - 3)"""
    out = set()
    for d in (-1, 0, 1):
        idn = rnd(s * k) + d
        out.add((k - min(max(idn, 2), k), False))
        if k >= GAP_MIN_K:
            n = len(sid_sites(k, True)[0])
            out.add((k - GAP - min(max(idn, k - GAP - n), k - GAP), True))
    return sorted(out)


def _sid_block(rng, k, variants, flank=0):
    """one query (the core, optionally inside `flank` residues of fq on either side) and one target per variant"""
    p0 = base_params()
    core = _rnd(rng, k)
    ln = letters()
    seqs, pairs = [_flanked(core, ln["fq"], flank, k + 2 * flank)], []
    for m, gapped in variants:
        sites, p = sid_sites(k, gapped)
        pos = rng.choice(sites, m, replace=False) if m else np.zeros(0, np.int64)
        ta = core[1].copy()
        ta[pos] = (ta[pos] + rng.integers(1, 20, m).astype(np.uint8)) % 20          # another letter
        cols = _columns(core, (core[0], ta))
        t = (core[0], ta)
        score = cols.sum()
        if gapped:
            keep = np.ones(k, bool); keep[p:p + GAP] = False
            t = (core[0][keep], ta[keep])
            score = cols[keep].sum() - (p0.gap_open + (GAP - 1) * p0.gap_ext)
        w = _want(score, flank, 0, k, len(t[0]), k - m - (GAP if gapped else 0), 1 if gapped else 0)
        w["aln_len"] = k
        i = len(seqs)
        seqs.append(t)
        tag = "idents=%d%s" % (w["idents"], " gapped" if gapped else "")
        pairs += [(0, i, tag, w), (i, 0, tag + " swapped", _swapped(w))]
    return seqs, pairs


def _eval_block(rng, k, lx, ly):
    core = _rnd(rng, k)
    x, y = int(rng.integers(0, lx - k + 1)), int(rng.integers(0, ly - k + 1))
    ln = letters()
    w = _want(_columns(core, core).sum(), x, y, k, k, k, 0)
    return [_flanked(core, ln["fq"], x, lx), _flanked(core, ln["ft"], y, ly)], [(0, 1, "(Lq,Lt)=(%d,%d)" % (lx, ly), w), (1, 0, "(Lq,Lt)=(%d,%d)" % (ly, lx), _swapped(w))]


def _ovf_core(k):
    """a homopolymer of the best-scoring residue whose last 40 AA letters are the second-best: the reversed query then scores less than
    the query, so the corrected score stays positive"""
    ln = letters()
    return _cat(_rep(ln["best"], k - 40), _rep(ln["second"], 40))


def _lands(seqs, pairs):
    """the scalar oracle's record of every pair at threshold 1 -> the reversed-query scores, or None if one differs from the intent"""
    O, p = _O(), base_params()
    odb = O.OracleDb(s3=[s[0] for s in seqs], sa=[s[1] for s in seqs])
    revs = []
    for q, t, _, w in pairs:
        r = O.align_pair(odb, p, q, t, 1)
        if int(r["pass_evalue"]) != 1 or int(r["score_rev"]) <= 0 or any(int(r[f]) != w[f] for f in w):
            return None
        revs.append(int(r["score_rev"]))
    return revs


@functools.lru_cache(maxsize=None)
def _block(kind, *key):
    """the block (kind, key) of the first attempt that lands -> (seqs, pairs, reversed-query scores, attempt)"""
    for attempt in range(64):
        rng = np.random.default_rng([KINDS.index(kind), attempt] + [int(1000 * x) for x in key])
        if kind == "span":
            seqs, pairs = _span_block(rng, *key)
        elif kind == "sid":
            seqs, pairs = _sid_block(rng, key[1], sid_variants(*key))
        elif kind == "eval":
            seqs, pairs = _eval_block(rng, *key[1:])
        elif kind == "long-sid":
            seqs, pairs = _sid_block(rng, key[1] - 20, sid_variants(key[0], key[1] - 20), flank=10)
        else:
            seqs, pairs = _span_block(rng, *key, core=_ovf_core(key[0]))
        revs = _lands(seqs, pairs)
        if revs is not None:
            return seqs, pairs, revs, attempt
    raise AssertionError("no attempt of block %s %s lands" % (kind, key))


KINDS = ("span", "sid", "eval", "long-sid", "ovf")


# ---- groups: one database and one hit list --------------------------------------------------------------------------------------------
class Group:
    """name, s3 / sa (lists of code arrays), pairs in hit-list order (dicts: q, t, lq, lt, family, label, want or None, rev), counts"""

    def __init__(self, name):
        self.name, self.s3, self.sa, self.pairs, self.attempts = name, [], [], [], 0

    def add(self, family, label, block):
        seqs, pairs = block[0], block[1]
        revs = block[2] if len(block) > 2 else [0] * len(pairs)
        self.attempts += block[3] if len(block) > 3 else 0
        base = len(self.s3)
        self.s3 += [s[0] for s in seqs]; self.sa += [s[1] for s in seqs]
        for (q, t, layout, w), rev in zip(pairs, revs):
            self.pairs.append(dict(q=base + q, t=base + t, lq=len(seqs[q][0]), lt=len(seqs[t][0]), family=family,
                                   label="%s %s %s" % (family, label, layout), want=w, rev=rev))

    def close(self):
        self.pairs.sort(key=lambda pr: pr["q"])          # stable: the hit lists, query by query
        self.q = np.array([pr["q"] for pr in self.pairs], np.uint32)
        self.t = np.array([pr["t"] for pr in self.pairs], np.uint32)
        self.counts = np.bincount(self.q, minlength=len(self.s3)).astype(np.uint32)
        # the mirror of pair i (the same two sequences in the other direction), and whether i is the direction the engine computes
        # (the shorter query; equal lengths: the smaller id)
        at = {(pr["q"], pr["t"]): i for i, pr in enumerate(self.pairs)}
        assert len(at) == len(self.pairs), "a hit list names a target once"
        for pr in self.pairs:
            pr["mirror"] = at.get((pr["t"], pr["q"]))
            pr["rep"] = (pr["lq"], pr["q"]) < (pr["lt"], pr["t"])
        return self


def cov_grid(c):
    """(k, L): L over the grid, k = round(c L) + {-1, 0, 1} clipped to 3 <= k <= L"""
    out = []
    for L in sorted(set(GRID_L + (EXTRA_L_HALF if c == 0.5 else ()))):          # (110 is on the grid already)
        out += [(k, L) for k in sorted({min(max(rnd(c * L) + d, 3), L) for d in (-1, 0, 1)})]
    return out


def _add_spans(g, family, c):
    for k, L in cov_grid(c):
        g.add(family, "c=%s (k=%d, L=%d)" % (c, k, L), _block("span", k, L))


@functools.lru_cache(maxsize=None)
def cov_group(c):
    g = Group("cov-%s" % c)
    _add_spans(g, "cov", c)
    return g.close()


@functools.lru_cache(maxsize=None)
def len_group(c):
    """the grid read as sequence lengths: the related trios (known spans) and two unrelated random sequences per grid point, both
    directions; one sequence of a single residue against 1, 2 and 5 residues"""
    g = Group("len-%s" % c)
    _add_spans(g, "len-related", c)
    seqs, ids, pairs = [], {}, []

    def seq(which, n):
        if (which, n) not in ids:
            ids[(which, n)] = len(seqs)
            seqs.append(_rnd(np.random.default_rng([90 + which, n]), n))
        return ids[(which, n)]
    for k, L in cov_grid(c) + [(1, 1), (1, 2), (1, 5)]:
        a, b = seq(0, k), seq(1, L)
        pairs += [(a, b, "c=%s (Lq,Lt)=(%d,%d)" % (c, k, L), None), (b, a, "c=%s (Lq,Lt)=(%d,%d)" % (c, L, k), None)]
    g.add("len-unrelated", "", (seqs, pairs))
    return g.close()


@functools.lru_cache(maxsize=None)
def sid_group(s):
    g = Group("sid-%s" % s)
    for k in SID_K:
        g.add("sid", "s=%s k=%d" % (s, k), _block("sid", s, k))
    return g.close()


EVAL_SHAPES = ((40, 60, 50), (90, 120, 100), (150, 200, 160))          # (k, Lx, Ly): every coverage is at least 0.66
EVAL_STEPS = ("corrected", "corrected+1", "score", "score+1")


@functools.lru_cache(maxsize=None)
def eval_group():
    """identical-core pairs (X, Y) in both directions; pair number 16 s + 4 a + b of shape s gets the table entries a for X and b for Y"""
    g = Group("eval")
    for s, (k, lx, ly) in enumerate(EVAL_SHAPES):
        for ab in range(16):
            g.add("eval", "X:%s Y:%s" % (EVAL_STEPS[ab // 4], EVAL_STEPS[ab % 4]), _block("eval", 16 * s + ab, k, lx, ly))
    return g.close()


def eval_table(kind):
    """--min-score-table of the eval group, one threshold per sequence: `mixed` as described at eval_group, `none` 30,000 for everyone
    (nothing reaches it: only the forward pass runs)"""
    g = eval_group()
    tab = np.full(len(g.s3), 30000, np.int32)
    if kind == "mixed":
        for pr in g.pairs:
            w = pr["want"]
            ab = (pr["q"] // 2) % 16
            step = ab // 4 if pr["q"] % 2 == 0 else ab % 4
            tab[pr["q"]] = (w["score"] - pr["rev"], w["score"] - pr["rev"] + 1, w["score"], w["score"] + 1)[step]
    return tab


LONG_L, LONG_C, LONG_S = 2060, 0.8, 0.9
OVF_L, OVF_C = 2000, 0.85


@functools.lru_cache(maxsize=None)
def long_group():
    """queries of 2,060 residues (the long-query kernel): spans 1,647 .. 1,649 of 2,060 against 0.8; a core of 2,040 between two flanks of
    10 with 1,835 .. 1,837 identities against 0.9, with and without the deletion.  The other direction of each pair has a query of at most
    2,048 residues, so the one-call run computes the shared DP in a packed class and the per-query run meets both kernels"""
    g = Group("route-long")
    for d in (-1, 0, 1):
        k = rnd(LONG_C * LONG_L) + d
        g.add("cov", "c=%s (k=%d, L=%d)" % (LONG_C, k, LONG_L), _block("span", k, LONG_L))
    g.add("sid", "s=%s k=%d" % (LONG_S, LONG_L), _block("long-sid", LONG_S, LONG_L))
    return g.close()


@functools.lru_cache(maxsize=None)
def ovf_group():
    """cores of 1,699 .. 1,701 best-scoring residues (19 per column: 32,201 and more) inside 2,000 residues: the packed kernels report an
    overflow and the pair is re-run in int32; 1,700 / 2,000 against 0.85"""
    g = Group("route-ovf")
    for d in (-1, 0, 1):
        k = rnd(OVF_C * OVF_L) + d
        g.add("cov", "c=%s (k=%d, L=%d)" % (OVF_C, k, OVF_L), _block("ovf", k, OVF_L))
    return g.close()


# ---- option sets: what the GPU test runs and the CPU test proves the expectation for ----------------------------------------------------
class OptSet:
    """opts: the options oracle and engine share; extra: execution choices of the engine alone; table: None, "mixed" or "none" (eval)"""

    def __init__(self, name, group, c, mode=0, sid=0.0, len_gate=0, table=None, extra=""):
        self.name, self.group, self.c, self.mode, self.sid, self.len_gate, self.table, self.extra = name, group, c, mode, sid, len_gate, table, extra

    def opts(self):
        s = "-c %s --cov-mode %d" % (self.c, self.mode)
        if self.sid:
            s += " --min-seq-id %s" % self.sid
        if self.len_gate:
            s += " --length-gate 1"
        return s if self.table else E1 + " " + s

    def __repr__(self):
        return self.name


def _sets():
    out = {"cov": [], "len": [], "sid": [], "eval": [], "routes": []}
    for c in COV_THRESHOLDS:
        out["cov"] += [OptSet("cov-%s-mode%d" % (c, m), functools.partial(cov_group, c), c, m) for m in (0, 1, 2)]
    for c in LEN_THRESHOLDS:
        out["len"] += [OptSet("len-%s-mode%d" % (c, m), functools.partial(len_group, c), c, m, len_gate=1) for m in (0, 1, 2)]
    out["len"].append(OptSet("len-gate-off-under-c0", functools.partial(len_group, 0.8), 0.0, 0, len_gate=1))
    out["sid"] = [OptSet("sid-%s" % s, functools.partial(sid_group, s), 0.5, 0, sid=s) for s in SID_THRESHOLDS]
    out["sid"].append(OptSet("sid-0.9-backtraces", functools.partial(sid_group, 0.9), 0.5, 0, sid=0.9, extra="-a"))
    out["eval"] = [OptSet("eval-mixed-mode%d" % m, eval_group, 0.5, m, table="mixed") for m in (0, 2)] + [OptSet("eval-none", eval_group, 0.5, 0, table="none")]
    i32 = "--sw-kernel i32"
    out["routes"] = [OptSet("i32-cov-0.8", functools.partial(cov_group, 0.8), 0.8, 0, extra=i32),
                     OptSet("i32-len-0.8", functools.partial(len_group, 0.8), 0.8, 0, len_gate=1, extra=i32),
                     OptSet("i32-sid-0.9", functools.partial(sid_group, 0.9), 0.5, 0, sid=0.9, extra=i32),
                     OptSet("i32-eval-mixed", eval_group, 0.5, 0, table="mixed", extra=i32)]
    out["routes"] += [OptSet("long-cov-%s-mode%d" % (LONG_C, m), long_group, LONG_C, m) for m in (0, 1, 2)]
    out["routes"].append(OptSet("long-sid-%s" % LONG_S, long_group, 0.5, 0, sid=LONG_S))
    out["routes"] += [OptSet("ovf-cov-%s-mode%d" % (OVF_C, m), ovf_group, OVF_C, m) for m in (0, 1, 2)]
    return out


OPTION_SETS = _sets()
ALL_SETS = [o for fam in OPTION_SETS.values() for o in fam]


# ---- the closed form ------------------------------------------------------------------------------------------------------------------
def _by_mode(mode, q_ok, t_ok):
    return (q_ok and t_ok) if mode == 0 else t_ok if mode == 1 else q_ok


def length_gate_lets_through(o, lq, lt):
    """rule UC-1/L: cov_mode 0 both quotients, 1 Lq / Lt, 2 Lt / Lq; off under -c 0"""
    if not o.len_gate or not o.c > 0:
        return True
    return lq > 0 and lt > 0 and _by_mode(o.mode, f32_ge(lt, lq, o.c), f32_ge(lq, lt, o.c))


def thresholds(o, g):
    """the E-value threshold of every sequence as a query: the table's entry, or 1"""
    return eval_table(o.table) if o.table else np.ones(len(g.s3), np.int32)


def expected(o, pr, thr):
    """the record of pair `pr` under option set `o` with E-value threshold `thr` for its query, from the intended integers alone (pr["rev"],
    the full reversed-query score, is the one number taken from the oracle).  None: the pair has no intent (unrelated sequences) and the
    length gate lets it through - only the oracle knows its record"""
    rec = dict.fromkeys(FIELDS, 0)
    if not length_gate_lets_through(o, pr["lq"], pr["lt"]):
        return rec                                   # not aligned: the all-zero record
    w = pr["want"]
    if w is None:
        return None
    rec["score"] = w["score"]
    rec["score_rev"] = pr["rev"] if w["score"] >= thr else 0          # UC-1.1
    rec["corrected"] = rec["score"] - rec["score_rev"]
    rec["pass_evalue"] = int(rec["score"] > 0 and rec["corrected"] >= thr)
    rec.update(qstart=-1, qend=-1, tstart=-1, tend=-1)
    if not rec["pass_evalue"]:
        return rec
    rec.update({f: w[f] for f in ("qstart", "qend", "tstart", "tend")})
    ok = _by_mode(o.mode, f32_ge(w["qend"] - w["qstart"] + 1, pr["lq"], o.c), f32_ge(w["tend"] - w["tstart"] + 1, pr["lt"], o.c))
    if ok and o.sid > 0:
        rec.update(aln_len=w["aln_len"], idents=w["idents"], gap_opens=w["gap_opens"])
        ok = f32_ge(w["idents"], w["aln_len"], o.sid)
    rec["accepted"] = int(ok)
    return rec


def normalised(rec):
    """positions are defined only for pairs that pass the E-value gate: -1 elsewhere - except in the all-zero record of a pair that was
    not aligned, which stays as it is"""
    r = {f: int(rec[f]) for f in FIELDS}
    if not r["pass_evalue"] and any(r.values()):
        r.update(qstart=-1, qend=-1, tstart=-1, tend=-1)
    return r


@functools.lru_cache(maxsize=None)
def _oracle_records(name):
    o = next(x for x in ALL_SETS if x.name == name)
    O, g = _O(), o.group()
    p = util.oracle_params(O, o.opts())
    odb = O.OracleDb(s3=g.s3, sa=g.sa)
    thr = thresholds(o, g)
    return [normalised(O.align_pair(odb, p, pr["q"], pr["t"], int(thr[pr["q"]]))) for pr in g.pairs]


def oracle_records(o):
    """the scalar oracle's record of every pair of the option set's group, in hit-list order; computed once per session"""
    return _oracle_records(o.name)
