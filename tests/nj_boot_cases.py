"""The shared case list of rule UC-N/B (bootstrap support) for test_nj_boot.py (host twins) and test_nj_boot_gpu.py (HIP kernels):
draws, alignments with their replicate sets for the counts, batches of matrices for the joins, hand cases for support and the labelled line.
Everything is seeded; the references (nj_boot_ref.py over nj_ref.py) are computed once per process and shared."""
import functools
import random

import numpy as np

import nj_boot_ref as BR
import nj_cases as NC
import nj_ref as R

SEED = 0x5EED0B007
DRAW_WIDTHS = (1, 2, 3, 255, 256, 257, 2 ** 31 - 1)      # the last: the first 64 draws only
DRAW_SEEDS = (0, 1, 2 ** 64 - 1)
DRAW_REPS = (0, 1, 99999)
REP_SETS = ((0, 1), (5, 3), (0, 8))                       # (rep0, n_rep)


def count_shapes(T, C):
    return [(n, w) for n in (2, 3, T - 1, T, T + 1, 2 * T + 2) for w in (1, 3, C - 1, C, C + 1, 2 * C + 3)]


@functools.lru_cache(maxsize=None)
def shape_rows(n, w):
    return tuple(NC.random_rows(random.Random(n * 7919 + w), n, w))


def content_rows():
    """the contents the counts must not trip over: every byte value, a row of gaps only, lower against upper case"""
    hand = NC.hand_rows()
    return {k: hand[k] for k in ("every_byte", "all_gap_row", "lower_against_upper")}


@functools.lru_cache(maxsize=None)
def reference_counts(rows, seed, b):
    """(comp, diff) of replicate b: nj_ref's counts of the explicitly resampled rows"""
    return BR.replicate_counts(list(rows), seed, b)


def gathered(rows, cols):
    """the rows of a replicate, gathered with numpy: what uc_nj_counts is fed in the check that does not go through the reference"""
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)
    return np.ascontiguousarray(a[:, np.asarray(cols, np.int64)])


# ---- matrices for the batched joins
JOIN_SIZES = (4, 5, 6, 63, 64, 65)                        # and L - 1, L, L + 1, 257, 1030 (two replicates) once L is known


def join_sizes(L):
    return [(n, 3) for n in JOIN_SIZES + (L - 1, L, L + 1, 257)] + [(1030, 2)]


@functools.lru_cache(maxsize=None)
def replicate_alignment(n):
    return tuple(NC.evolved_rows(random.Random(4000 + n), n, 96, rate=0.2))


def stacked_join_cases():
    """n -> (names, [B][n][n], the reference's join dicts): nj_cases.join_cases() grouped by size, so that ties (equal_n), additive and non-metric
    matrices take their different paths inside one batch"""
    groups = {}
    for name, (D, want) in sorted(NC.join_cases().items()):
        if len(D) >= 3:
            groups.setdefault(len(D), []).append((name, D, want))
    return {n: ([g[0] for g in v], np.stack([g[1] for g in v]), [g[2] for g in v]) for n, v in groups.items()}


def one_of(batch, b):
    return {k: v[b] for k, v in batch.items()}


# ---- support and the labelled line, by hand
def caterpillar(n):
    """n >= 4: the join dict of ((((0,1),2),3) ... with unit lengths: join s joins node n + s - 1 (leaf 0 for s = 0) with leaf s + 1"""
    steps = n - 3
    ja = [0] + [n + s - 1 for s in range(1, steps)]
    jb = [s + 1 for s in range(steps)]
    root = [n + steps - 1, n - 2, n - 1]
    return {"join_a": ja, "join_b": jb, "len_a": [1.0] * steps, "len_b": [1.0] * steps, "root_node": root, "root_len": [1.0, 1.0, 1.0]}


FOUR_AB = {"join_a": [0], "join_b": [1], "len_a": [0.1], "len_b": [0.2], "root_node": [4, 2, 3], "root_len": [0.05, 0.3, 0.4]}      # ab | cd
FOUR_AC = {"join_a": [0], "join_b": [2], "len_a": [0.1], "len_b": [0.2], "root_node": [4, 1, 3], "root_len": [0.05, 0.3, 0.4]}      # ac | bd
FOUR_CD = {"join_a": [2], "join_b": [3], "len_a": [0.1], "len_b": [0.2], "root_node": [4, 0, 1], "root_len": [0.05, 0.3, 0.4]}      # cd | ab: the same split as ab | cd


def fasta_of(names, rows):
    return "".join(">%s\n%s\n" % (n, r.decode("latin-1")) for n, r in zip(names, rows))
