"""The shared case list of rule UC-N for test_nj.py (host twins) and test_nj_gpu.py (HIP kernels): alignments for the counts,
count pairs for the transform, matrices for the joins, names for the Newick writer.  Everything is seeded; the references (nj_ref.py) are computed
once per process and shared."""
import functools
import random

import numpy as np

import nj_ref as R

AA = b"ACDEFGHIKLMNPQRSTVWY"


def random_rows(rng, n, w, gap=0.08, x=0.03, lower=0.05, alphabet=AA):
    rows = []
    for _ in range(n):
        r = bytearray(rng.choice(alphabet) for _ in range(w))
        for c in range(w):
            u = rng.random()
            if u < gap:
                r[c] = ord("-")
            elif u < gap + x:
                r[c] = ord("X")
            elif u < gap + x + lower:
                r[c] = r[c] | 0x20
        rows.append(bytes(r))
    return rows


def evolved_rows(rng, n, w, rate=0.15):
    """sequences evolved down a random tree (a row is a mutated copy of an earlier row), with gaps and X sprinkled in"""
    rows = [bytearray(rng.choice(AA) for _ in range(w))]
    while len(rows) < n:
        child = bytearray(rows[rng.randrange(len(rows))])
        for c in range(w):
            if rng.random() < rate:
                child[c] = rng.choice(AA)
        rows.append(child)
    out = []
    for r in rows:
        r = bytearray(r)
        for c in range(w):
            u = rng.random()
            if u < 0.06:
                r[c] = ord("-")
            elif u < 0.08:
                r[c] = rng.choice(b"Xx")
        out.append(bytes(r))
    return out


def count_shapes(T, C):
    """the shapes around the tile height T and the LDS column chunk C"""
    return [(n, w) for n in (2, 3, T - 1, T, T + 1, 2 * T + 1) for w in (1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3)]


@functools.lru_cache(maxsize=None)
def count_cases(T, C):
    """name -> (rows, (comp, diff) of the reference)"""
    cases = {}
    for n, w in count_shapes(T, C):
        rows = random_rows(random.Random(n * 100003 + w), n, w)
        if w >= 2:                                  # the last column alone tells the first two rows apart
            rows[1] = rows[0][:-1] + (b"A" if rows[0][-1:] != b"A" else b"C")
        cases["shape_%dx%d" % (n, w)] = rows
    for name, rows in hand_rows().items():
        cases[name] = rows
    for seed in range(6):
        rng = random.Random(7000 + seed)
        cases["campaign_%d" % seed] = evolved_rows(rng, rng.randrange(4, 40), rng.randrange(40, 600))
    return {k: (v, R.counts(v)) for k, v in cases.items()}


def hand_rows():
    every = bytes(range(256))
    return {
        "all_gap_row": [b"ACDEFGHIKL", b"----------", b"ACDEFGHIKM"],
        "lower_against_upper": [b"ACDEFGHIKL", b"acdefghikl", b"aCdEfGhIkM"],
        "x_star_dot_0_255": [b"AX*.\x00\xffxA-A", b"AAAAAAAAAA", b"AX*.\x00\xffxC-C", b"X*.\x00\xff.*x-X"],
        "identical_rows": [b"MKVLAAGIW", b"MKVLAAGIW", b"MKVLAAGIW"],
        "differ_everywhere": [b"AAAAAAAAAAAAA", b"CCCCCCCCCCCCC", b"DDDDDDDDDDDDD"],
        "last_column_only": [b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNP", b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNQ"],
        "every_byte": [every, every[::-1], bytes((b + 1) & 255 for b in every)],
        "brackets_beside_letters": [b"@AZ[`az{", b"@az[`AZ{", b"AAAAAAAA"],
    }


def hand_counts():
    """name -> (comp, diff) written out by hand"""
    return {
        "all_gap_row": ([0, 10, 0], [0, 1, 0]),
        "lower_against_upper": ([10, 10, 10], [0, 1, 1]),
        # row 0 is informative at columns 0, 7 (the x at 6 is not), 9; row 3 nowhere
        "x_star_dot_0_255": ([3, 3, 0, 3, 0, 0], [0, 2, 0, 2, 0, 0]),
        "identical_rows": ([9, 9, 9], [0, 0, 0]),
        "differ_everywhere": ([13, 13, 13], [13, 13, 13]),
        "last_column_only": ([33], [1]),
        "brackets_beside_letters": ([4, 4, 4], [0, 2, 2]),
    }


def distance_cases():
    """name -> (comp, diff, n): triangles of n rows"""
    pairs = [(0, 0), (1, 0), (1, 1), (10000, 8541), (10000, 8542), (10000, 8489), (10000, 8490), (10000, 8491), (10000, 8492), (7, 3), (1000, 1),
             (100, 50), (3, 1), (2 ** 31 - 1, 2 ** 30), (2 ** 31 - 1, 0)]
    rng = random.Random(5)
    more = []
    for _ in range(21):
        c = rng.randrange(1, 5000)
        more.append((c, rng.randrange(0, c + 1)))
    return {"edges": ([p[0] for p in pairs], [p[1] for p in pairs], 6), "random": ([p[0] for p in more], [p[1] for p in more], 7)}


# ---- matrices for the joins
def random_matrix(rng, n):
    """points on a line plus noise: symmetric, non-negative, zero diagonal, no tree metric"""
    x = [rng.random() * 4 for _ in range(n)]
    D = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            D[i, j] = D[j, i] = abs(x[i] - x[j]) + rng.random()
    return D


def random_tree(rng, n):
    """an unrooted binary tree on the leaves 0 .. n - 1 with edge lengths k / 8 (k = 1 .. 16): a list of (u, v, length); inner nodes from n"""
    edges = [(0, n, rng.randrange(1, 17) / 8), (1, n, rng.randrange(1, 17) / 8), (2, n, rng.randrange(1, 17) / 8)] if n >= 3 else [(0, 1, rng.randrange(1, 17) / 8)]
    nxt = n + 1
    for leaf in range(3, n):
        k = rng.randrange(len(edges))
        u, v, _ = edges[k]
        edges[k] = (u, nxt, rng.randrange(1, 17) / 8)
        edges.append((nxt, v, rng.randrange(1, 17) / 8))
        edges.append((leaf, nxt, rng.randrange(1, 17) / 8))
        nxt += 1
    return edges


def tree_metric(edges, n):
    """leaf-to-leaf path lengths of a tree given as (u, v, length) edges: n x n, exact for multiples of 1/8"""
    adj = {}
    for u, v, l in edges:
        adj.setdefault(u, []).append((v, l))
        adj.setdefault(v, []).append((u, l))
    D = np.zeros((n, n))
    for s in range(n):
        dist, stack = {s: 0.0}, [s]
        while stack:
            u = stack.pop()
            for v, l in adj[u]:
                if v not in dist:
                    dist[v] = dist[u] + l
                    stack.append(v)
        for t in range(n):
            D[s, t] = dist[t]
    return D


def edges_of_joins(n, j):
    """the tree of a join dict as (u, v, length) edges; the root is node n + steps"""
    edges, steps = [], len(j["join_a"])
    for s in range(steps):
        edges.append((int(j["join_a"][s]), n + s, float(j["len_a"][s])))
        edges.append((int(j["join_b"][s]), n + s, float(j["len_b"][s])))
    for t in range(2 if n == 2 else 3):
        edges.append((int(j["root_node"][t]), n + steps, float(j["root_len"][t])))
    return edges


def additive_cases():
    out = {}
    for n in (2, 3, 4, 5, 9, 64, 65):
        out["additive_%d" % n] = tree_metric(random_tree(random.Random(900 + n), n), n)
    return out


EQUAL_5 = {"join_a": [0, 5], "join_b": [1, 2], "len_a": [0.5, 0.0], "len_b": [0.5, 0.5], "root_node": [6, 3, 4], "root_len": [0.0, 0.5, 0.5]}


@functools.lru_cache(maxsize=None)
def join_cases():
    """name -> (D, the reference's join dict)"""
    cases = {}
    for n in (2, 3, 4, 5, 64, 65, 200):
        cases["random_%d" % n] = random_matrix(random.Random(300 + n), n)
    for n in (2, 3, 4, 5, 9):
        cases["equal_%d" % n] = np.ones((n, n)) - np.eye(n)
    cases.update(additive_cases())
    # d(0, 1) is small while row 0 is near everything and row 1 far from everything: l0 = 0.5 * 0.1 + (2.1 - 18.1) / 4 < 0
    cases["clamp"] = np.array([[0, 0.1, 1, 1], [0.1, 0, 9, 9], [1, 9, 0, 1], [1, 9, 1, 0]], np.float64)
    dup = random_matrix(random.Random(77), 8)
    dup[3, :] = dup[5, :]; dup[:, 3] = dup[:, 5]; dup[3, 3] = dup[5, 5] = dup[3, 5] = dup[5, 3] = 0.0
    cases["duplicate_rows"] = dup
    cases["all_zero"] = np.zeros((6, 6))
    for name, (rows, (comp, diff)) in count_cases_small().items():
        cases["campaign_" + name] = np.array(R.distances(comp, diff, len(rows)))
    return {k: (v, R.join(v.tolist())) for k, v in cases.items()}


@functools.lru_cache(maxsize=None)
def count_cases_small():
    """the campaign's alignments (the joins run on their matrices too); independent of the kernel's geometry"""
    out = {}
    for seed in range(6):
        rng = random.Random(7000 + seed)
        rows = evolved_rows(rng, rng.randrange(4, 40), rng.randrange(40, 600))
        out["%d" % seed] = (rows, R.counts(rows))
    return out


@functools.lru_cache(maxsize=None)
def route_cases(L):
    """name -> D for the single entry point on both sides of the batch's LDS route (L rows and L + 1), at the smallest trees (4 has one step) and at 257, the
    first n where a row of pairs takes a second stride of 256 threads and the row sums a second workgroup.  Per size a tree metric, the all-zero
    matrix (every Q equal: the index tie-break alone decides, across waves and across partials) and a matrix with duplicated rows"""
    cases = {}
    for n in (4, 5, L, L + 1, 257):
        cases["tree_%d" % n] = tree_metric(random_tree(random.Random(1100 + n), n), n)
        cases["zero_%d" % n] = np.zeros((n, n))
        dup = random_matrix(random.Random(1200 + n), n)
        for a, b in ((1, n - 1), (n // 2, n - 2), (0, n // 3 + 1)):      # n = 4: rows 1 and 3, rows 0 and 2
            if a != b:
                dup[a, :] = dup[b, :]; dup[:, a] = dup[:, b]; dup[a, a] = dup[b, b] = dup[a, b] = dup[b, a] = 0.0
        cases["duplicate_rows_%d" % n] = dup
    return cases


NEWICK_NAMES = ["plain", "with space", "a:b", "it's", "(paren)", "semi;colon", "comma,", "[brack]", "tab\there", "Homo_sapiens.1"]


def same_joins(a, b, what=""):
    """join dicts: integers equal, fp64 by their bits"""
    for k in ("join_a", "join_b", "root_node"):
        assert [int(x) for x in a[k]] == [int(x) for x in b[k]], (what, k, list(a[k])[:8], list(b[k])[:8])
    for k in ("len_a", "len_b", "root_len"):
        x, y = np.ascontiguousarray(a[k], np.float64).view(np.uint64), np.ascontiguousarray(b[k], np.float64).view(np.uint64)
        assert np.array_equal(x, y), (what, k, list(a[k])[:8], list(b[k])[:8])
