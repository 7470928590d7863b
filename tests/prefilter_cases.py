"""Case builders and references for the kernel-level prefilter tests (tests/test_prefilter_cases.py on the CPU, tests/test_prefilter_kernels_gpu.py
on the device).  A case is a list of 3Di code arrays, an option string and the facts its test relies on; the amino-acid track plays no part in E1-E4
and is all zero.  Two references: the oracle's E1-E4 one query at a time with its stage counters (oracle_prefilter), and for homopolymers the closed
form of spec UC-1 in plain Python integers (hom_closed_form), which owes nothing to the oracle's code.

Run as a program (`python prefilter_cases.py OUT.npz`) it is the child process of test_merge_sorted_in_both_settings: UC_MERGE_SORTED is read once
per process, so each setting needs a process of its own."""
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")

import util      # noqa: E402

HOM = 2                      # letter D: 6 * S3[D][D] >= kmer_thr at -s 4 under the shipped stand-in matrix (asserted by the tests, not assumed)
ALL = "--min-ungapped-score 0 --max-seqs 1000"       # E4 drops nothing: every candidate is listed and its diag is the d* of E2
X = 20
COUNTERS = ("n_sim_kmers", "n_kmer_hits", "n_candidates", "n_prefilter_hits")


def pattern_offsets(p):
    pat = p.pattern.decode()
    return [i for i, c in enumerate(pat) if c == "1"], len(pat)


def valid_kmer_positions(seq, offs, span):
    """start positions of the k-mers without an X"""
    return [i for i in range(0, len(seq) - span + 1) if all(seq[i + o] < 20 for o in offs)]


# ---------------------------------------------------------------- references
_ORACLE_CACHE = {}


def oracle_prefilter(O, s3, opts, key=None):
    """E1-E4 of every query by uco_prefilter_query with a Counts struct per query, over a pool of at most 16 threads (the call releases the GIL).
    -> dict(cnt u32[n], hits list of HIT_DTYPE arrays, per_query list of counter dicts, totals dict, seconds).  `key` caches the result for the
    session: the reference of a case is computed once and shared."""
    if key is not None and (key, opts) in _ORACLE_CACHE:
        return _ORACLE_CACHE[(key, opts)]
    p = util.oracle_params(O, opts)
    odb = O.OracleDb(s3=s3, sa=[np.zeros(len(x), np.uint8) for x in s3])
    t0 = time.time()
    ix = O.build_index(odb, p)
    n, M = odb.n, p.max_seqs
    L = O.lib()

    def one(q):
        c = O.Counts()
        buf = np.zeros(M, O.HIT_DTYPE)
        k = L.uco_prefilter_query(C.byref(odb.db), C.byref(ix), q, C.byref(p), buf.ctypes.data, C.byref(c))
        return k, buf[:k].copy(), {f: int(getattr(c, f)) for f in COUNTERS}

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as pool:
        res = list(pool.map(one, range(n)))
    O.free_index(ix)
    out = dict(cnt=np.array([r[0] for r in res], np.uint32), hits=[r[1] for r in res], per_query=[r[2] for r in res],
               totals={f: sum(r[2][f] for r in res) for f in COUNTERS}, seconds=time.time() - t0, params=p)
    if key is not None:
        _ORACLE_CACHE[(key, opts)] = out
    return out


def hom_cnt(nq, nt, d):
    """k-mer hits of a homopolymer pair on diagonal d (nq, nt k-mer positions)"""
    return max(0, min(nq, nt, nq - d, nt + d))


def hom_closed_form(lengths, sdiag, span, min_diag_hits, min_ungapped, max_seqs):
    """Spec UC-1 on homopolymers of ONE letter whose k-mer is similar to itself and to nothing else in the index, in plain integers: every query k-mer
    position hits every target position, cnt(d) = min(nq, nt, nq - d, nt + d), d* = min(0, Lq - Lt) (most hits, then the smallest diagonal), the
    ungapped score is min(255, sdiag * overlap(d*)).  -> (lists: per query [(target, score, diag)] in list order, n_kmer_hits, n_candidates)"""
    lists, n_hits, n_cand = [], 0, 0
    for Lq in lengths:
        nq, cand = Lq - span + 1, []
        for t, Lt in enumerate(lengths):
            nt = Lt - span + 1
            if nq < 1 or nt < 1:
                continue
            n_hits += nq * nt
            best = max(hom_cnt(nq, nt, d) for d in range(-(nt - 1), nq))
            dstar = min(d for d in range(-(nt - 1), nq) if hom_cnt(nq, nt, d) == best)
            assert dstar == min(0, Lq - Lt) and best == min(nq, nt)
            if best < min_diag_hits:
                continue
            n_cand += 1
            overlap = min(Lq, Lt + dstar) - max(dstar, 0)
            score = min(255, sdiag * overlap)
            if score >= min_ungapped:
                cand.append((t, score, dstar))
        cand.sort(key=lambda r: (-r[1], r[0]))
        lists.append(cand[:max_seqs])
    return lists, n_hits, n_cand


def exact_diagonal_counts(q, t, offs, span):
    """hits of EXACT k-mer matches of one pair per diagonal -> dict diagonal -> count (a small numpy count, no similar k-mers)"""
    def kmers(s):
        n = len(s) - span + 1
        v = np.zeros(max(n, 0), np.int64)
        for m, o in enumerate(offs):
            v += s[o:o + n].astype(np.int64) * 20 ** m
        return v
    kq, kt = kmers(np.asarray(q)), kmers(np.asarray(t))
    i, j = np.nonzero(kq[:, None] == kt[None, :])
    d, c = np.unique(i - j, return_counts=True)
    return dict(zip(d.tolist(), c.tolist()))


# ---------------------------------------------------------------- case families
def hom(lengths, letter=HOM):
    return [np.full(L, letter, np.uint8) for L in lengths]


SWEEP_LENGTHS = list(range(10, 34)) + list(range(58, 90))       # family 1: group sizes 1 .. 6400, run lengths 1 .. 80, boundaries at every offset mod 64
SWEEP_LONG = list(range(58, 90))
SWEEP_OPTS = ("-c 0.8 --min-diag-hits 1 " + ALL, "-c 0.8 " + ALL)      # plain expansion (expand_kernel) / the double-hit filter (filter_kernel)


def extreme_lengths(lmax, n):
    """family 2: n homopolymer lengths with one k-mer only (10) first, the longest (lmax) in the middle, the n - 2 lengths just below lmax around it"""
    rest = list(range(lmax - (n - 2), lmax))
    return [10] + rest[: n // 2] + [lmax] + rest[n // 2:]


EXTREME_SETS = ((64, 32), (65, 33), (64, 33), (65, 32))          # (longest, count): dbits 7 / 8 x tbits 5 / 6


def tandem_repeats(seed=7):
    """family 3: periods 7 and 13 over one random unit each, lengths 100 .. 300 in steps of 9 (46 sequences), every sequence starting at its own phase"""
    rng = np.random.default_rng(seed)
    s3 = []
    for period in (7, 13):
        unit = rng.integers(0, 20, period, dtype=np.uint8)
        for k, L in enumerate(range(100, 301, 9)):
            s3.append(np.tile(unit, L // period + 3)[k % period: k % period + L].copy())
    return s3


REPEAT_OPTS = "-c 0.8 " + ALL


def longest_pair(seed=3):
    """family 4: two random sequences of 65,535 residues that share a 40-residue block at opposite ends, and the block alone"""
    rng = np.random.default_rng(seed)
    block = rng.integers(0, 20, 40, dtype=np.uint8)
    a, b = rng.integers(0, 20, 65535, dtype=np.uint8), rng.integers(0, 20, 65535, dtype=np.uint8)
    a[:40] = block
    b[-40:] = block
    return [a, b, block.copy()]


LONGEST_OPTS = "-c 0.8"


def tied_copies(seed=5):
    """family 5: 45 exact copies of one random 120-residue sequence and 10 unrelated ones, in a seeded order -> (s3, ids of the copies ascending).
    Sequence 0 is a copy: the E4 key of (score 255, target 0) has an all-zero low half, the one value at which a comparison of a whole key with
    a query's bare key field turns on < against <= (rank_flag_kernel)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 20, 120, dtype=np.uint8)
    order = rng.permutation(55)
    order = np.concatenate([[0], order[order != 0]])
    s3 = [None] * 55
    for k, pos in enumerate(order):
        s3[pos] = base.copy() if k < 45 else rng.integers(0, 20, 120, dtype=np.uint8)
    return s3, sorted(int(x) for x in order[:45])


def loaded_filter(O, seed=11, n_targets=60, lt=400, lq=2000):
    """family 7: reduced-alphabet sequences over the three letters with the largest diagonal score: targets of lt residues and one query of lq (last)"""
    p = O.default_params()
    top = sorted(range(20), key=lambda a: (-p.S3[a * 21 + a], a))[:3]
    rng = np.random.default_rng(seed)
    letters = np.array(top, np.uint8)
    return [letters[rng.integers(0, 3, lt)] for _ in range(n_targets)] + [letters[rng.integers(0, 3, lq)]]


LOADED_OPTS = "-c 0.8 " + ALL


def saturating_filter(O, seed=13, n_targets=1400, lt=80, lq=2000, n_letters=5):
    """family 7, bitmap saturation: many short random targets and one long query (last) over the five letters with the largest diagonal score, so
    that the query's hits fall on more than 2^19 DISTINCT (target, diagonal) keys - more keys than either LDS bitmap of filter_kernel has bits"""
    p = O.default_params()
    top = sorted(range(20), key=lambda a: (-p.S3[a * 21 + a], a))[:n_letters]
    rng = np.random.default_rng(seed)
    letters = np.array(top, np.uint8)
    return [letters[rng.integers(0, n_letters, lt)] for _ in range(n_targets)] + [letters[rng.integers(0, n_letters, lq)]]


SATURATING_OPTS = "-c 0.8 --min-ungapped-score 0 --max-seqs 2000"


def query_keys(O, s3, q, opts):
    """the k-mer hits of query q as (target, diagonal) pairs: a numpy count over similar_kmers against a sorted k-mer index, independent of the oracle's
    E2 loop -> (hits, distinct (target, diagonal) keys)"""
    p = util.oracle_params(O, opts)
    offs, span = pattern_offsets(p)

    def kmers(x):
        n = len(x) - span + 1
        if n <= 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        v, ok = np.zeros(n, np.int64), np.ones(n, bool)
        for m, o in enumerate(offs):
            c = np.asarray(x[o:o + n], np.int64)
            v += c * 20 ** m
            ok &= c < 20
        return v[ok], np.nonzero(ok)[0]
    kv, kt, kp = [], [], []
    for t, x in enumerate(s3):
        v, pos = kmers(x)
        kv.append(v); kt.append(np.full(len(v), t, np.int64)); kp.append(pos)
    kv, kt, kp = np.concatenate(kv), np.concatenate(kt), np.concatenate(kp)
    order = np.argsort(kv, kind="stable")
    kv, kt, kp = kv[order], kt[order], kp[order]
    qv, qpos = kmers(s3[q])
    memo, keys = {}, []
    for v, i in zip(qv.tolist(), qpos.tolist()):
        if v not in memo:
            letters = [(v // 20 ** m) % 20 for m in range(6)]
            sim = np.sort(O.similar_kmers(letters, p.kmer_thr, p).astype(np.int64))
            lo, hi = np.searchsorted(kv, sim, "left"), np.searchsorted(kv, sim, "right")
            memo[v] = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi) if b > a] or [np.zeros(0, np.int64)]).astype(np.int64)
        e = memo[v]
        keys.append(kt[e] * (1 << 20) + (i - kp[e] + (1 << 17)))
    keys = np.concatenate(keys)
    return len(keys), len(np.unique(keys))


def query_runs(O, s3, q, opts):
    """non-empty index ranges ("runs") of query q: (query position, similar k-mer that occurs in the index) pairs, and the k-mer hits they hold"""
    p = util.oracle_params(O, opts)
    offs, span = pattern_offsets(p)
    occ = {}
    for s in s3:
        for i in valid_kmer_positions(s, offs, span):
            v = sum(int(s[i + o]) * 20 ** m for m, o in enumerate(offs))
            occ[v] = occ.get(v, 0) + 1
    runs = hits = 0
    memo = {}
    for i in valid_kmer_positions(s3[q], offs, span):
        letters = tuple(int(s3[q][i + o]) for o in offs)
        if letters not in memo:
            sim = O.similar_kmers(letters, p.kmer_thr, p)
            present = [occ[int(v)] for v in sim if int(v) in occ]
            memo[letters] = (len(present), sum(present))
        runs += memo[letters][0]
        hits += memo[letters][1]
    return runs, hits


def distinct_kmer_runs(O, s3, opts):
    """runs of the DISTINCT k-mers of all queries (what UC_DRUN_MAX budgets)"""
    p = util.oracle_params(O, opts)
    offs, span = pattern_offsets(p)
    occ = set()
    for s in s3:
        for i in valid_kmer_positions(s, offs, span):
            occ.add(tuple(int(s[i + o]) for o in offs))
    vals = {sum(c * 20 ** m for m, c in enumerate(k)) for k in occ}
    return sum(sum(1 for v in O.similar_kmers(k, p.kmer_thr, p) if int(v) in vals) for k in occ)


X_VARIANTS = ("plain", "x_first", "x_last", "x_every10", "x_none_valid")


def with_x(seq, variant):
    """family 8: an X at position 0, at the last k-mer's last letter, at every 10th residue, and at residues 0, 4 and 8 of every ten.  Under the
    spaced pattern 1101010011 (offsets 0 1 3 5 8 9 of a span of 10) an X at every 10th residue still leaves the k-mers that start at residues 3, 4, 6
    and 8 of every ten (the X falls on a position the pattern skips); the last variant is the one that leaves no valid k-mer at all."""
    s = np.array(seq, np.uint8)
    if variant == "x_first":
        s[0] = X
    elif variant == "x_last":
        s[-1] = X
    elif variant == "x_every10":
        s[::10] = X
    elif variant == "x_none_valid":
        s[0::10] = X
        s[4::10] = X
        s[8::10] = X
    return s


def x_cases():
    """-> {name: (s3, variant of every sequence, opts)}: family 1 and family 3 sequences in every X variant.  The homopolymers are 20 .. 44 residues
    long: at 5 points per residue their ungapped scores stay below the saturation at 255, so an X inside the overlap shows in the compared score"""
    homs = [(s, v) for L in range(20, 46, 2) for v in X_VARIANTS for s in [with_x(np.full(L, HOM, np.uint8), v)]]
    reps = [(with_x(s, v), v) for s in tandem_repeats()[::4] for v in X_VARIANTS]
    return {"x_hom": ([s for s, _ in homs], [v for _, v in homs], "-c 0.8 --min-diag-hits 1 " + ALL),
            "x_rep": ([s for s, _ in reps], [v for _, v in reps], REPEAT_OPTS)}


# ---------------------------------------------------------------- the engine side (GPU tests and the child process)
def run_engine(s3, opts, env=None):
    """Engine(opts).set_db -> prefilter -> (counts, hits, stats) with the environment variables `env` set for the duration of the run"""
    import unicore_amd as U
    off, c3, _ = util.flat(s3, s3)
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    e = U.Engine(opts, verbosity=1)
    try:
        e.set_db(off, c3, np.zeros(len(c3), np.uint8))
        e.reset_stats()
        e.prefilter()
        cnt, hits = e.hits()
        return cnt, hits, e.stats()
    finally:
        e.close()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


SWEEP_CHUNK_RES = "400"       # < 400 target k-mer positions per chunk: a homopolymer chunk stays under the engine's density limit of 400 hits per query residue
REPEAT_CHUNK_RES = "2400"


if __name__ == "__main__":      # child of test_merge_sorted_in_both_settings: chunked runs of families 1 and 3 under this process's UC_MERGE_SORTED
    out = {}
    for name, s3, opts, chunk in (("sweep", hom(SWEEP_LENGTHS), SWEEP_OPTS[0], SWEEP_CHUNK_RES), ("sweep_filter", hom(SWEEP_LENGTHS), SWEEP_OPTS[1], SWEEP_CHUNK_RES),
                                  ("repeat", tandem_repeats(), REPEAT_OPTS, REPEAT_CHUNK_RES)):
        cnt, hits, st = run_engine(s3, opts, {"UC_PREFILTER_CHUNK_RES": chunk})
        out[name + "_cnt"], out[name + "_hits"] = cnt, hits
        out[name + "_counters"] = np.array([st[k] for k in COUNTERS + ("n_filtered_hits",)], np.uint64)
    np.savez(sys.argv[1], **out)
