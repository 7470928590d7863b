"""Test-side reference of rule UC-1/G (--cluster-mode 2, greedy incremental): the sequential walk, in plain Python.
The product code never imports this."""
import numpy as np


def greedy_incremental(n, edges, lens):
    """nodes by length descending (ties: ascending id); an unassigned node becomes a representative and takes its unassigned neighbours"""
    adj = [[] for _ in range(n)]
    for a, b in np.asarray(edges, np.int64).reshape(-1, 2):
        if a != b:
            adj[a].append(int(b))
            adj[b].append(int(a))
    assign = [-1] * n
    for u in sorted(range(n), key=lambda i: (-int(lens[i]), i)):
        if assign[u] < 0:
            assign[u] = u
            for v in adj[u]:
                if assign[v] < 0:
                    assign[v] = u
    return np.array(assign, np.uint32)
