"""Graphs, length patterns and property checks shared by test_cluster_mode2.py (host variant) and test_cluster_mode2_gpu.py (device variant)."""
import numpy as np

SIZES = (1, 2, 7, 64, 257, 2000)
LENGTH_PATTERNS = ("equal", "ascending", "random")


def shapes(n, rng):
    """the graph shapes of test_gpu_parity.py::test_device_set_cover_equals_the_sequential_rule at n nodes"""
    ids = np.arange(n)
    s = {
        "empty": np.zeros((0, 2), np.uint32),
        "path": np.stack([ids[:-1], ids[1:]], 1),
        "ring": np.stack([ids, (ids + 1) % n], 1),
        "star": np.stack([np.zeros(n, int), ids], 1),
        "two stars sharing leaves": np.concatenate([np.stack([np.zeros(n // 2, int), ids[n // 2:n // 2 + n // 2]], 1),
                                                    np.stack([np.ones(n // 2, int), ids[n // 2:n // 2 + n // 2]], 1)]) if n > 4 else np.zeros((0, 2), int),
        "self + duplicates": np.concatenate([np.stack([ids, ids], 1), np.stack([ids[:-1], ids[1:]], 1), np.stack([ids[1:], ids[:-1]], 1)]),
        "descending path": np.stack([ids[1:][::-1], ids[:-1][::-1]], 1),
    }
    for k in range(6):
        m = int(rng.integers(0, 6 * n + 1))
        s["random %d" % k] = rng.integers(0, n, (m, 2))
    if n >= 64:
        fam = rng.integers(0, max(2, n // 12), n)
        s["cliques with bridges"] = np.array([(i, j) for i in range(n) for j in np.nonzero(fam == fam[i])[0][:9]] +
                                             [(int(a), int(b)) for a, b in rng.integers(0, n, (n // 10, 2))])
        s["hub chain"] = hub_chain(n)
    return {k: np.asarray(v, np.uint32).reshape(-1, 2) for k, v in s.items()}


def hub_chain(n):
    hubs = np.arange(0, n, 16)
    return np.concatenate([np.stack([hubs[:-1], hubs[1:]], 1)] + [np.stack([np.full(15, h), np.arange(h + 1, h + 16) % n], 1) for h in hubs])


def lengths(n, pattern, rng):
    if pattern == "equal":
        return np.full(n, 5, np.uint32)
    if pattern == "ascending":
        return (1 + np.arange(n)).astype(np.uint32)
    if pattern == "random":
        return rng.integers(1, 301, n).astype(np.uint32)
    raise ValueError(pattern)


def hub_chain_late_lengths(n):
    """Lengths for hub_chain(n) under which a representative of LOWER rank is decided in a LATER parallel round than one of higher rank.
    Hubs k = 0, 1, 2 of every four are long and descend along the chain (k: representative at once, k + 1: its member, k + 2: a representative
    only in round 2, when k + 1 is known to be a member).  Hub k + 3 is the shortest node of all and its leaves are mid-sized: the leaves are
    representatives in round 1 and make hub k + 3 a member in round 1, but hub k + 3 belongs to hub k + 2, which outranks the leaves."""
    ln = np.full(n, 40, np.uint32)
    hubs = np.arange(0, n, 16)
    for k, h in enumerate(hubs):
        if k % 4 == 3:
            ln[h] = 1
            ln[np.arange(h + 1, h + 16) % n] = 100
        else:
            ln[h] = 1000 - k
    for k, h in enumerate(hubs):          # the wrapped leaves of the last hub must not overwrite a hub
        ln[h] = 1 if k % 4 == 3 else 1000 - k
    return ln


def check_properties(n, edges, lens, assign, tag=None):
    """representatives are pairwise non-adjacent; every member is adjacent to its representative; no member outranks its representative"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    a = np.asarray(assign, np.int64)
    ids = np.arange(n)
    assert a.shape == (n,) and (a < n).all(), tag
    rep = a == ids
    assert rep[a].all(), (tag, "a representative's representative is itself")
    assert not (rep[e[:, 0]] & rep[e[:, 1]]).any(), (tag, "adjacent representatives")
    keys = set((e[:, 0] * n + e[:, 1]).tolist()) | set((e[:, 1] * n + e[:, 0]).tolist())
    mem = ids[~rep]
    assert all(int(v) * n + int(a[v]) in keys for v in mem), (tag, "a member is not adjacent to its representative")
    ln = np.asarray(lens, np.int64)
    assert ((ln[a[mem]] > ln[mem]) | ((ln[a[mem]] == ln[mem]) & (a[mem] < mem))).all(), (tag, "a member outranks its representative")
