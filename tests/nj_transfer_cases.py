"""The shared case list of rule UC-N/T (transfer bootstrap support) for test_nj_transfer.py (host twin) and test_nj_transfer_gpu.py
(HIP kernels): tree shapes as join records.  A tree is first a rooted binary nesting of leaves (a leaf is an int, a node a pair), then the join
records a neighbour joining would have written for it: one join per internal node in post-order, but for the root and one of its children, whose
three neighbours stay at the trifurcation.  Everything is seeded; the references (nj_transfer_ref.py) are computed once per process and shared."""
import functools
import random

import numpy as np

import nj_transfer_ref as TR


def joins_of(tree, n):
    """the join dict (unit lengths) of a rooted binary nesting on leaves 0 .. n - 1, n >= 3"""
    left, right = tree
    if isinstance(left, int):
        left, right = right, left
    assert not isinstance(left, int), "three leaves at least"
    ja, jb = [], []

    def emit(t):      # post-order without recursion: a caterpillar of 16,384 leaves is a long way down
        stack, done = [(t, 0)], []
        while stack:
            x, st = stack.pop()
            if isinstance(x, int):
                done.append(x)
            elif st == 0:
                stack.append((x, 1)); stack.append((x[1], 0)); stack.append((x[0], 0))
            else:
                b, a = done.pop(), done.pop()
                ja.append(a); jb.append(b)
                done.append(n + len(ja) - 1)
        return done.pop()

    root = [emit(left[0]), emit(left[1]), emit(right)]
    steps = n - 3
    assert len(ja) == steps
    return {"join_a": ja, "join_b": jb, "len_a": [1.0] * steps, "len_b": [1.0] * steps, "root_node": root, "root_len": [1.0, 1.0, 1.0]}


def caterpillar(n, order=None):
    order = list(range(n)) if order is None else order
    t = (order[0], order[1])
    for v in order[2:]:
        t = (t, v)
    return t


def balanced(n, order=None):
    level = list(range(n)) if order is None else list(order)
    while len(level) > 1:
        level = [(level[k], level[k + 1]) if k + 1 < len(level) else level[k] for k in range(0, len(level), 2)]
    return level[0]


def random_tree(n, seed):
    """a random join order: two of the nodes still without a parent, drawn uniformly, until one is left"""
    rng, nodes = random.Random(seed), list(range(n))
    while len(nodes) > 1:
        a = nodes.pop(rng.randrange(len(nodes)))
        b = nodes.pop(rng.randrange(len(nodes)))
        nodes.append((a, b))
    return nodes[0]


def regrafted(tree, n, seed):
    """the tree with one leaf pruned and regrafted on another branch: every split of the old tree is in the new one up to that leaf"""
    rng = random.Random(seed)
    v = rng.randrange(n)

    def prune(t):
        stack, done = [(t, 0)], []
        while stack:
            x, st = stack.pop()
            if isinstance(x, int):
                done.append(x)
            elif st == 0:
                stack.append((x, 1)); stack.append((x[1], 0)); stack.append((x[0], 0))
            else:
                b, a = done.pop(), done.pop()
                done.append(b if a == v else a if b == v else (a, b))
        return done.pop()

    rest = prune(tree)
    count = 2 * (n - 1) - 1      # the nodes of the pruned tree, in post-order
    at, seen = rng.randrange(count), [0]

    def graft(t):
        stack, done = [(t, 0)], []
        while stack:
            x, st = stack.pop()
            if isinstance(x, int) or st == 1:
                if st == 1:
                    b, a = done.pop(), done.pop()
                    x = (a, b)
                done.append((x, v) if seen[0] == at else x)
                seen[0] += 1
            else:
                stack.append((x, 1)); stack.append((x[1], 0)); stack.append((x[0], 0))
        return done.pop()

    return graft(rest)


def shuffled(n, seed):
    order = list(range(n))
    random.Random(seed).shuffle(order)
    return order


@functools.lru_cache(maxsize=None)
def case(n, n_rep=6):
    """(main, replicates) as join dicts on n >= 4 leaves: the main tree is a random join order; the replicates are, in turn, a copy of the main tree
    (every phi 0), the main tree with one leaf regrafted (every phi <= 1), an unrelated random tree, a caterpillar and a balanced tree over shuffled
    leaves (every true distance of a deep split is large: only the cap, or a padded row taken for a split, can undercut it), another regraft"""
    main_tree = random_tree(n, 1000 + n)
    kinds = [main_tree, regrafted(main_tree, n, 7 * n), random_tree(n, 5000 + n), caterpillar(n, shuffled(n, n)), balanced(n, shuffled(n, n + 1)), regrafted(main_tree, n, 11 * n)]
    reps = [joins_of(kinds[k % len(kinds)] if k < len(kinds) else random_tree(n, 9000 + n + k), n) for k in range(n_rep)]
    return joins_of(main_tree, n), reps


@functools.lru_cache(maxsize=None)
def shaped_case(n, shape):
    """a main tree of one shape against replicates of the others"""
    trees = {"caterpillar": caterpillar(n), "balanced": balanced(n), "random": random_tree(n, 31 * n)}
    others = [trees[k] for k in sorted(trees) if k != shape] + [caterpillar(n, shuffled(n, 3 * n)), regrafted(trees[shape], n, n + 5), trees[shape]]
    return joins_of(trees[shape], n), [joins_of(t, n) for t in others]


@functools.lru_cache(maxsize=None)
def reference(n, n_rep=6, first=None):
    """(phi, light) of case(n, n_rep) from the plain-Python rule; first: only that many replicates (n^2 set operations each)"""
    main, reps = case(n, n_rep)
    return TR.transfer(n, main, reps[:first])


def arrays(reps):
    return np.array([r["join_a"] for r in reps], np.uint32).reshape(len(reps), -1), np.array([r["join_b"] for r in reps], np.uint32).reshape(len(reps), -1)


# the hand example of the rule: N = 7, the main split {a, b, c}
HAND_NAMES = list("abcdefg")
HAND_MAIN = joins_of(((((0, 1), 2), 3), ((4, 5), 6)), 7)            # splits ab, abc, ef, abcd
HAND_HOLDS = joins_of(((((0, 1), 2), 3), ((4, 5), 6)), 7)           # holds abc: phi 0
HAND_AB_ONLY = joins_of(((((0, 1), 3), 2), ((4, 5), 6)), 7)         # ab, abd, ef, abcd: abc is one leaf from ab (and from abcd)
HAND_ABD = joins_of((((((0, 3), 1), 4), 2), (5, 6)), 7)             # ad, abd, abde, fg: the nearest to abc are at h = 2, the cap
