"""Rule UC-1/R (--cluster-reassign) restated in plain Python, for tests/test_cluster_reassign*.py and tests/golden/make_clust_reassign.py.

Everything that is computed comes from the CPU oracle (oracle_py: align_pair, min_score, OracleDb.subset, prefilter_shard, the workflow) except
the final clustering of the edge list, which is the host uc_cluster_graph (tested on its own in test_cluster_mode2.py).  No device is needed.

  1 verify     every member x of A against its representative: align_pair(query = A[x], target = x) in the full database
  2 seeds      D' = representatives (ascending) ++ rejected members (ascending)
  3 re-search  the rejected members as queries against D' (prefilter at the final sensitivity, then align_pair in D', E-value against D')
  4 re-cluster the graph {A[x], x} of the members that passed + the accepted pairs of 3 under the run's clustering rule
"""
import numpy as np

import ungapped_all_ref as X


def split_options(opts):
    """an option string of uc_cluster -> (the part util.oracle_params understands, dict of the workflow / rule switches)"""
    tok, base, sw = opts.split(), [], dict(cluster_mode=0, prefilter_mode=0, single_step=False, reassign=False, sens=4.0)
    i = 0
    while i < len(tok):
        f = tok[i]
        if f in ("--cluster-reassign", "--single-step-clustering"):
            on = True
            if i + 1 < len(tok) and tok[i + 1] in ("0", "1"):
                on = tok[i + 1] == "1"
                i += 1
            sw["reassign" if f == "--cluster-reassign" else "single_step"] = on
            i += 1
            continue
        if f == "--cluster-mode":
            sw["cluster_mode"] = 2 if int(tok[i + 1]) in (2, 3) else int(tok[i + 1])
        elif f == "--prefilter-mode":
            sw["prefilter_mode"] = int(tok[i + 1])
        else:
            if f == "-s":
                sw["sens"] = float(tok[i + 1])
            base += tok[i:i + 2]
        i += 2
    return " ".join(base), sw


def workflow_assign(O, odb, p, sw, threads=4):
    """the assignment the workflow leaves WITHOUT the flag (set cover in every round): the plain step or pre-step + 3-step cascade"""
    if sw["single_step"]:
        return O.cluster(odb, p, threads=threads, dumps=False)["assign"]
    return O.cluster_workflow(odb, p, O.cascade_thresholds(p, sw["sens"], 3), linclust_m=20, threads=threads)["assign"]


def accepted(O, odb, p, q, t):
    return int(O.align_pair(odb, p, q, t, O.min_score(odb, p, q))["accepted"]) == 1


def research_lists(O, sub, p, q0, prefilter_mode):
    """hit lists (targets in list order) of the queries [q0, sub.n) against all of `sub`"""
    m = sub.n
    if prefilter_mode == 1:
        off = sub.offsets().astype(np.int64)
        c3, _ = sub.codes()
        s3 = [c3[off[i]:off[i + 1]] for i in range(m)]
        qs, ts = list(range(q0, m)), list(range(m))
        sc, dg = X.dense(O, s3, p, qs, ts)
        lists = X.hit_lists(sc, dg, ts, p.min_ungapped, p.max_seqs, lens=np.diff(off), queries=qs)
        return [[h[0] for h in l] for l in lists]
    cnt, hits = O.prefilter_shard(sub, p)
    return [[int(t) for t in hits[q, : cnt[q]]["t"]] for q in range(q0, m)]


def reassign(O, U, odb, p, A, cluster_mode=0, prefilter_mode=0):
    """rule UC-1/R on the assignment A.  Returns dict(assign, rejected [n] bool, counts = (verified, rejected, accepted re-search pairs
    without self pairs, final clusters), edges [k, 2])"""
    A = np.asarray(A, np.int64)
    n = odb.n
    assert len(A) == n and np.array_equal(A[A], A)
    rej = np.zeros(n, bool)
    edges = []
    members = [x for x in range(n) if A[x] != x]
    for x in members:
        if accepted(O, odb, p, int(A[x]), x):
            edges.append((int(A[x]), x))
        else:
            rej[x] = True
    R = [x for x in range(n) if A[x] == x]
    W = [x for x in range(n) if rej[x]]
    n_re = 0
    if W:
        ids = np.array(R + W, np.int64)
        sub = odb.subset(ids)
        for k, lst in enumerate(research_lists(O, sub, p, len(R), prefilter_mode)):
            q = len(R) + k
            for t in lst:
                if accepted(O, sub, p, q, t) and q != t:
                    edges.append((int(ids[q]), int(ids[t])))
                    n_re += 1
    ed = np.array(edges, np.uint32).reshape(-1, 2)
    lens = np.diff(odb.offsets().astype(np.int64)).astype(np.uint32)
    assign = U.cluster_graph(n, ed, lens, cluster_mode)
    return dict(assign=assign, rejected=rej, edges=ed, reps=R, research=W,
                counts=(len(members), len(W), n_re, int((assign == np.arange(n)).sum())))


def unaccepted_members(O, odb, p, res):
    """the rule's consequence, checked pair by pair with the oracle: every member of the final assignment has an accepted alignment with its
    representative in one of the two directions, in the full database (step 1) or, with a rejected sequence as the query, in D' (step 3).
    Returns the members for which that fails (expected: none)."""
    assign, R, W = res["assign"], res["reps"], res["research"]
    ids = R + W
    loc = {g: i for i, g in enumerate(ids)}
    sub = odb.subset(np.array(ids, np.int64)) if W else None
    bad = []
    for x in range(odb.n):
        r = int(assign[x])
        if r == x:
            continue
        ok = accepted(O, odb, p, r, x) or accepted(O, odb, p, x, r)
        for q, t in ((x, r), (r, x)):
            if not ok and sub is not None and q in loc and t in loc and loc[q] >= len(R):
                ok = accepted(O, sub, p, loc[q], loc[t])
        if not ok:
            bad.append(x)
    return bad
