"""Rule UC-N/T (transfer bootstrap support of the tree builder `nj`; TBE, Lemoine et al., Nature 2018) in plain Python on top of
nj_boot_ref.py: a split is the set of leaves below a join, the transfer distance of two splits is counted on the sets themselves (no bit tricks),
the transfer index is the smallest distance to any join of the replicate, capped at light - 1, and the label is the percentage of
1 - phi_sum / (B (light - 1)) rounded half up, in integers.  The library's host twin and HIP kernels are compared against this bit for bit."""
import nj_boot_ref as BR
import nj_ref as R


def leaf_sets(n, joins):
    """join s -> the frozenset of leaves below node n + s"""
    below, out = {i: frozenset([i]) for i in range(n)}, []
    for s in range(len(joins["join_a"])):
        L = below[int(joins["join_a"][s])] | below[int(joins["join_b"][s])]
        below[n + s] = L
        out.append(L)
    return out


def light(n, joins):
    return [min(len(L), n - len(L)) for L in leaf_sets(n, joins)]


def delta(n, x, y):
    """the transfer distance of two splits given by one side each: the leaves on which the sides differ, or those on which they agree"""
    h = len(x) + len(y) - 2 * len(x & y)      # |x symmetric-difference y|
    return min(h, n - h)


def phi_of(n, main, replicate):
    """the transfer index of every join of the main tree in one replicate"""
    mine, theirs = leaf_sets(n, main), leaf_sets(n, replicate)
    assert len(mine) == len(theirs) == max(n - 3, 0)
    return [min([len(x) - 1 if 2 * len(x) <= n else n - len(x) - 1] + [delta(n, x, y) for y in theirs]) for x in mine]


def transfer(n, main, replicates):
    """(phi [B][n - 3], light [n - 3])"""
    return [phi_of(n, main, r) for r in replicates], light(n, main)


def labels(phi, li, B):
    out = []
    for s, l in enumerate(li):
        den, total = B * (l - 1), sum(p[s] for p in phi)
        assert 0 <= total <= den
        out.append((200 * (den - total) + den) // (2 * den))
    return out


def newick(names, joins, li, phi_sum, B):
    """nj_ref.newick with UC-N/T's label of node N + s between its `)` and its `:`"""
    if not B or len(names) <= 3:
        return R.newick(names, joins)
    N = len(names)
    lab = [(200 * (B * (l - 1) - int(p)) + B * (l - 1)) // (2 * B * (l - 1)) for l, p in zip(li, phi_sum)]

    def sub(v):
        out, stack = [], [(v, 0)]
        while stack:
            x, st = stack.pop()
            if x < N:
                out.append(R.quote(names[x]))
                continue
            s = x - N
            if st == 0:
                out.append("(")
                stack.append((x, 1)); stack.append((joins["join_a"][s], 0))
            elif st == 1:
                out.append(":%.6f," % joins["len_a"][s])
                stack.append((x, 2)); stack.append((joins["join_b"][s], 0))
            else:
                out.append(":%.6f)%d" % (joins["len_b"][s], lab[s]))
        return "".join(out)

    return "(" + ",".join("%s:%.6f" % (sub(int(joins["root_node"][t])), joins["root_len"][t]) for t in range(3)) + ");\n"


def transfer_of_fasta(text, B, seed, model="kimura"):
    """everything uc_tree_infer_support writes in mode tbe: {"nwk", "support" (the replicates that hold the split), "light", "phi_sum", "labels",
    "boottrees", "tsv" (the dump's boot.tsv)}"""
    names, rows = R.read_fasta(text)
    n = len(rows)
    comp, diff = R.counts(rows)
    main = R.join(R.distances(comp, diff, n, model))
    reps = [BR.replicate_tree(rows, seed, b, model) for b in range(B)]
    out = {"boottrees": "".join(R.newick(names, r) for r in reps)}
    if n <= 3 or not B:
        out.update(nwk=R.newick(names, main), support=[], light=[], phi_sum=[], labels=[], tsv="")
        return out
    phi, li = transfer(n, main, reps)
    phi_sum = [sum(p[s] for p in phi) for s in range(n - 3)]
    sup = [sum(p[s] == 0 for p in phi) for s in range(n - 3)]
    assert sup == BR.support(n, main, reps)
    lab = labels(phi, li, B)
    out.update(nwk=newick(names, main, li, phi_sum, B), support=sup, light=li, phi_sum=phi_sum, labels=lab,
               tsv="".join("%d\t%d\t%d\t%d\t%d\n" % (s, sup[s], li[s], phi_sum[s], lab[s]) for s in range(n - 3)))
    return out
