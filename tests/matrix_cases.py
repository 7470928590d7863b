"""Case builders for the tests under custom substitution matrices and k-mer patterns (tests/test_matrix_cases.py on the CPU,
tests/test_custom_matrices_gpu.py and tests/test_prefilter_matrices_gpu.py on the device).  A matrix case is a pair of 21 x 21 integer arrays
(3Di track, amino-acid track) in the letter order of util.LET + "X", written to files in the format load_matrix reads and handed to the engine and
to the oracle as THE SAME files (--mat3di / --mat-aa).  Every builder is seeded and deterministic.

  directed          S(a, b) = S(a, a) and S(b, a) = min(S) for three 3Di letter pairs and one amino-acid pair: a sequence rich in `a` letters aligns
                    to its copy with every a replaced by b at its self score, and the copy aligns back far lower
  perturbed         the shipped matrices with +-3 on the 3Di upper triangle and +-2 on the amino-acid one: nearly every score is direction dependent
  only_s3 / only_sa the perturbation on one track, the other untouched (a symmetry check that looks at one track misses one of them)
  hot               every 3Di diagonal entry 48: the best score five letters can still add is 240 for every k-mer
  mixed_hot         eight 3Di diagonal entries 48: only k-mers rich in those letters pass 191
  negative          every 3Di off-diagonal entry -48 and ten letters with the diagonal entry -25 as well (whole rows <= -25): the derived --k-score is
                    -63, and k-mers with three of those letters among their first five have a NEGATIVE best remaining score, below -64, while
                    still similar to themselves.  (The threshold has to be the derived one: a negative --k-score means "not given" to the
                    engine, and under a threshold >= 0 no k-mer whose first five letters add less than -64 can pass with a sixth of at most 48.)

`rest5` below is the quantity the similar-k-mer search of uc_kmer_match.hip keeps per DFS level: the sum of the row maxima of the k-mer's letters that
the levels behind the first one decide, i.e. of its first five letters in pattern order."""
import os

import numpy as np

import util

HOT_LETTERS = (2, 3, 4, 5, 6, 7, 8, 9)         # mixed_hot: D E F G H I K L
NEG_LETTERS = tuple(range(10))                 # negative: A C D E F G H I K L
DIRECTED_3DI = ((0, 1), (2, 3), (4, 5))        # (a, b) = (A, C), (D, E), (F, G)
DIRECTED_AA = ((0, 1),)                        # (A, C)
X = 20


def base(O):
    """the shipped stand-in 3Di matrix and BLOSUM62 as the oracle loads them -> (S3, SA) int32 [21, 21]"""
    p = O.default_params()
    return np.array(p.S3[:], np.int32).reshape(21, 21), np.array(p.SA[:], np.int32).reshape(21, 21)


def write_matrix(path, M):
    letters = util.LET + "X"
    with open(path, "w") as f:
        f.write("# test matrix (tests/matrix_cases.py)\n")
        f.write("   " + " ".join("%3s" % c for c in letters) + "\n")
        for a, c in enumerate(letters):
            f.write(c + "  " + " ".join("%3d" % int(v) for v in M[a]) + "\n")
    return path


def _directed(M, pairs):
    M = M.copy()
    lo = int(M[:20, :20].min())
    for a, b in pairs:
        M[a, b] = M[a, a]
        M[b, a] = lo
    return M


def _perturb(M, amp, seed):
    M = M.copy()
    rng = np.random.default_rng(seed)
    iu = np.triu_indices(20, 1)
    M[iu] = np.clip(M[iu] + rng.integers(-amp, amp + 1, len(iu[0])), -48, 48)
    return M


def matrices(O, name):
    """-> (S3, SA) of the case `name`"""
    S3, SA = base(O)
    if name == "directed":
        return _directed(S3, DIRECTED_3DI), _directed(SA, DIRECTED_AA)
    if name == "perturbed":
        return _perturb(S3, 3, 101), _perturb(SA, 2, 102)
    if name == "only_s3":
        return _perturb(S3, 3, 101), SA
    if name == "only_sa":
        return S3, _perturb(SA, 2, 102)
    if name == "hot":
        S3[np.arange(20), np.arange(20)] = 48
        return S3, SA
    if name == "mixed_hot":
        for a in HOT_LETTERS:
            S3[a, a] = 48
        return S3, SA
    if name == "negative":
        d = np.diag(S3).copy()
        S3[:20, :20] = -48
        S3[np.arange(20), np.arange(20)] = d[:20]
        for a in NEG_LETTERS:
            S3[a, a] = -25
        return S3, SA
    raise KeyError(name)


NAMES = ("directed", "perturbed", "only_s3", "only_sa", "hot", "mixed_hot", "negative")


def write_case(O, name, tmp_dir):
    """write the two files of case `name` -> (S3, SA, option string "--mat3di PATH --mat-aa PATH")"""
    S3, SA = matrices(O, name)
    m3 = write_matrix(os.path.join(str(tmp_dir), name + "_3di.out"), S3)
    ma = write_matrix(os.path.join(str(tmp_dir), name + "_aa.out"), SA)
    return S3, SA, "--mat3di %s --mat-aa %s" % (m3, ma)


# ---------------------------------------------------------------- databases
def _replace(x, pairs):
    y = x.copy()
    for a, b in pairs:
        y[x == a] = b
    return y


def directed_db(seed=17, n_base=8):
    """n_base sequences of 60 .. 300 residues, half of their 3Di letters (a third of the amino acids) `a` letters of the directed pairs and none of
    them a `b` letter, each followed by its copy with every a replaced by b -> (s3, sa); base i is sequence 2 i, its copy 2 i + 1"""
    rng = np.random.default_rng(seed)
    a3, b3 = [a for a, _ in DIRECTED_3DI], [b for _, b in DIRECTED_3DI]
    aa, ba = [a for a, _ in DIRECTED_AA], [b for _, b in DIRECTED_AA]
    o3 = np.array([c for c in range(20) if c not in a3 + b3], np.uint8)
    oa = np.array([c for c in range(20) if c not in aa + ba], np.uint8)
    s3, sa = [], []
    for L in np.linspace(60, 300, n_base).astype(int):
        x3 = np.where(rng.random(L) < 0.5, rng.choice(a3, L), rng.choice(o3, L)).astype(np.uint8)
        xa = np.where(rng.random(L) < 0.33, rng.choice(aa, L), rng.choice(oa, L)).astype(np.uint8)
        s3 += [x3, _replace(x3, DIRECTED_3DI)]
        sa += [xa, _replace(xa, DIRECTED_AA)]
    return s3, sa


def family_case_db():
    """the database of the perturbed, hot, mixed-hot and negative cases"""
    return util.family_db(3, n_fam=6, members=4)


def rest5_plus_bias(s3, S3, pattern, bias=64):
    """bias + the sum of the row maxima of the first five letters (pattern order) of every valid k-mer of the database, and the sum over all six
    -> (int array [n_kmers] of bias + rest5, int array of rest6), in plain integers"""
    offs = [i for i, c in enumerate(pattern) if c == "1"]
    span = len(pattern)
    rowmax = S3[:20, :20].max(1)
    r5, r6 = [], []
    for s in s3:
        for i in range(0, len(s) - span + 1):
            c = [int(s[i + o]) for o in offs]
            if all(v < 20 for v in c):
                r5.append(bias + sum(int(rowmax[v]) for v in c[:5]))
                r6.append(sum(int(rowmax[v]) for v in c))
    return np.array(r5, np.int64), np.array(r6, np.int64)


# ---------------------------------------------------------------- the gapped sweep
# one query length per lane-group width of every class table of uc_sw_plan.hip, and the long-query kernel:
#   table 0: G = 16 up to 512 rows, 32 up to 1024, 64 beyond     table 1: 16 up to 384, 32 up to 768, 64 beyond
#   table 2: 16 up to 256, 32 up to 512, 64 beyond               table 3: 64 everywhere
SWEEP_QUERY_LENGTHS = (32, 64, 128, 448, 640, 896, 1280, 2049)
SWEEP_G = {0: {32: 16, 64: 16, 128: 16, 448: 16, 640: 32, 896: 32, 1280: 64}, 1: {32: 16, 64: 16, 128: 16, 448: 32, 640: 32, 896: 64, 1280: 64},
           2: {32: 16, 64: 16, 128: 16, 448: 32, 640: 64, 896: 64, 1280: 64}, 3: {L: 64 for L in (32, 64, 128, 448, 640, 896, 1280)}}


def _mutate_indel(rng, a3, aa, rate=0.15):
    b3, ba = a3.copy(), aa.copy()
    m = rng.random(len(b3)) < rate
    b3[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
    m = rng.random(len(ba)) < rate
    ba[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
    if len(b3) > 40:
        c = int(rng.integers(10, len(b3) // 2))
        b3, ba = np.delete(b3, slice(c, c + 3)), np.delete(ba, slice(c, c + 3))
        c = int(rng.integers(len(b3) // 2, len(b3) - 10))
        b3 = np.concatenate([b3[:c], rng.integers(0, 20, 4, dtype=np.uint8), b3[c:]])
        ba = np.concatenate([ba[:c], rng.integers(0, 20, 4, dtype=np.uint8), ba[c:]])
    return b3, ba


def sweep_db(seed=29):
    """-> (s3, sa, pairs [(q, t)], kinds): per query length a sequence rich in `a` letters with its directed copy (both ways round), a mutated copy
    with indels, a truncated copy and two unrelated targets; the base query has five pairs, its copy one (odd counts: a lone last slot)"""
    rng = np.random.default_rng(seed)
    a3 = [a for a, _ in DIRECTED_3DI]
    s3, sa, pairs, kinds = [], [], [], []

    def add(x3, xa):
        s3.append(np.ascontiguousarray(x3, np.uint8)); sa.append(np.ascontiguousarray(xa, np.uint8))
        return len(s3) - 1

    unrel = add(rng.integers(0, 20, 150, dtype=np.uint8), rng.integers(0, 20, 150, dtype=np.uint8))
    for L in SWEEP_QUERY_LENGTHS:
        x3 = np.where(rng.random(L) < 0.5, rng.choice(a3, L), rng.integers(0, 20, L)).astype(np.uint8)
        xa = np.where(rng.random(L) < 0.33, DIRECTED_AA[0][0], rng.integers(0, 20, L)).astype(np.uint8)
        q = add(x3, xa)
        c = add(_replace(x3, DIRECTED_3DI), _replace(xa, DIRECTED_AA))
        m = add(*_mutate_indel(rng, x3, xa))
        k = int(rng.integers(0, max(1, L // 3)))
        t = add(x3[k:k + max(20, L // 2)], xa[k:k + max(20, L // 2)])
        u = add(rng.integers(0, 20, L, dtype=np.uint8), rng.integers(0, 20, L, dtype=np.uint8))
        pairs += [(q, c), (c, q), (q, m), (q, t), (q, u), (q, unrel)]
        kinds += ["directed", "reverse", "mutated", "truncated", "unrelated", "unrelated"]
    return s3, sa, pairs, kinds


# ---------------------------------------------------------------- k-mer patterns
def pattern_sweep_lengths(span):
    """homopolymer lengths around the window edge j + span <= len: one residue short of a k-mer, exactly one k-mer, and up to 30 k-mer positions"""
    return list(range(span - 1, span + 30))


def with_x_for(seq, variant, pattern):
    """the X variants of prefilter_cases.with_x rebuilt for a pattern: "x_every" puts an X on every span-th residue starting at a position the
    pattern skips where there is one (k-mers survive) - under a contiguous pattern every k-mer holds one and none survives; "x_none_valid" puts an
    X on every residue with an even index, so that no window of 6 or more pattern letters is free of it"""
    span = len(pattern)
    s = np.array(seq, np.uint8)
    if variant == "x_first":
        s[0] = X
    elif variant == "x_last":
        s[-1] = X
    elif variant == "x_every":
        skipped = [i for i, c in enumerate(pattern) if c == "0"]
        s[(skipped[0] if skipped else 0)::span] = X
    elif variant == "x_none_valid":
        s[0::2] = X
    return s


PATTERN_X_VARIANTS = ("plain", "x_first", "x_last", "x_every", "x_none_valid")
