"""Cases for the way filter_kernel and expand_kernel (uc_kmer_filter.hip) find a query's runs in the plan of its super-batch: run r of a query belongs
to the last position whose run prefix is <= r and lies in the run list of that position's k-mer (tests/test_filter_runs_cases.py proves the shapes on
the CPU, tests/test_filter_runs_gpu.py runs them on the device).  References and the engine side are those of tests/prefilter_cases.py.

Cases A, C and D are random sequences over the TWO 3Di letters with the largest diagonal score: only 64 k-mers exist, every one of them occurs in the
database, and a position's run list is the set of the 64 that are similar to its k-mer - counted here by brute force (position_runs)."""
import itertools

import numpy as np

import prefilter_cases as PC
import util

TILE_RUNS = 2048                 # FILTER_RPT x FT of uc_kmer_filter.hip: runs per tile of filter_kernel
FILTER_PW = 1000                 # positions whose run prefix a filter workgroup holds in LDS; a longer query keeps every 2^sh-th
HIT_CAP_FLOOR = 1 << 20          # UC_HIT_CAP=1048576
OPTS = "-c 0.8 " + PC.ALL        # the double-hit filter (filter_kernel)
OPTS_PLAIN = "-c 0.8 --min-diag-hits 1 " + PC.ALL      # expand_kernel
A_LONG = 10                      # index of case A's long query: in the middle, so that it starts behind the first position of its batch


def two_letters(O):
    p = O.default_params()
    return sorted(range(20), key=lambda a: (-p.S3[a * 21 + a], a))[:2]


def _random(O, lengths, seed):
    rng = np.random.default_rng(seed)
    letters = np.array(two_letters(O), np.uint8)
    return [letters[rng.integers(0, 2, L)] for L in lengths]


A_LENGTHS = list(range(80, 90)) + [300] + list(range(90, 100))            # 21 sequences, 2,090 residues
D_LENGTHS = A_LENGTHS + list(range(100, 115))                             # case A enlarged by 15 sequences for the batch cuts of case D
A_CHUNK_RES = "1150"             # two target chunks of case A


def case_a(O):
    """A: 20 sequences of 80 .. 99 residues and one of 300 in the middle, whose 291 positions hold > 2,048 runs in lists of several runs each"""
    return _random(O, A_LENGTHS, 21)


def case_d(O):
    """D: case A (the same 21 sequences first) and 15 more of 100 .. 114 residues: > 3 x 2^20 k-mer hits, every query < 2^20"""
    return _random(O, D_LENGTHS, 21)


B_LENGTHS = [64, 66, 70, 2100, 65, 68]
B_LONG = 3


def case_b():
    """B: homopolymers; the one of 2,100 residues has 2,091 k-mer positions that all point at the one run list there is"""
    return PC.hom(B_LENGTHS)


C_DEAD = 2                       # case C's query without a valid k-mer, between two normal ones
C_GAPPED = (1, 3)


def case_c(O):
    """C: X residues at the start, in the middle (15 in a row: more zero-run positions than a k-mer spans) and at the end of two queries of 220 and 150
    residues, an all-X sequence between them, and plain sequences around"""
    s3 = _random(O, [90, 220, 40, 150, 95, 85], 22)
    for q in C_GAPPED:
        s3[q][:3] = PC.X
        s3[q][100:115] = PC.X
        s3[q][-2:] = PC.X
    s3[C_DEAD][:] = PC.X
    return s3


def position_runs(O, s3, opts):
    """-> per sequence an int array: the runs of every k-mer start position (0 where the k-mer holds an X, and behind the last k-mer), by brute force:
    the similar k-mers of the position's k-mer that occur anywhere in the database; and per sequence the k-mer hits of every position"""
    p = util.oracle_params(O, opts)
    offs, span = PC.pattern_offsets(p)
    occ = {}
    for s in s3:
        for i in PC.valid_kmer_positions(s, offs, span):
            k = tuple(int(s[i + o]) for o in offs)
            occ[k] = occ.get(k, 0) + 1
    val = {sum(c * 20 ** m for m, c in enumerate(k)): n for k, n in occ.items()}
    memo = {}
    runs, hits = [], []
    for s in s3:
        r, h = np.zeros(len(s), np.int64), np.zeros(len(s), np.int64)
        for i in PC.valid_kmer_positions(s, offs, span):
            k = tuple(int(s[i + o]) for o in offs)
            if k not in memo:
                present = [val[int(v)] for v in O.similar_kmers(list(k), p.kmer_thr, p) if int(v) in val]
                memo[k] = (len(present), sum(present))
            r[i], h[i] = memo[k]
        runs.append(r)
        hits.append(h)
    return runs, hits


def all_two_letter_kmers(O):
    return set(itertools.product(two_letters(O), repeat=6))


def target_chunks(lengths, chunk_res):
    """the target chunks the driver cuts at UC_PREFILTER_CHUNK_RES=chunk_res (prefilter_impl, uc_prefilter.hip) -> list of (first, end)"""
    chunks, b = [], 0
    while b < len(lengths):
        e, res = b, 0
        while e < len(lengths) and (e == b or res + lengths[e] <= chunk_res):
            res += lengths[e]
            e += 1
        chunks.append((b, e))
        b = e
    return chunks
