"""Rule UC-N/B (bootstrap support of the tree builder `nj`) in plain Python on top of nj_ref.py: the draws (SplitMix64's finaliser,
Python integers masked to 64 bits), a replicate as the explicitly resampled rows fed to nj_ref's counts / distances / join, splits as frozensets of
leaves, support by set equality, and the labelled Newick line.  The library's host twins and HIP kernels are compared against this bit for bit."""
import nj_ref as R

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
MIX_G = 0xE220A8397B1DCDAF      # the first output of SplitMix64 from state 0, as published with the generator


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, b):
    return mix(seed + G * (b + 1))


def column(W, seed, b, t):
    return (mix(key(seed, b) + G * (t + 1)) * W) >> 64


def columns(W, seed, b, count=None):
    """the first `count` (default: all W) draws of replicate b"""
    k = key(seed, b)
    return [(mix(k + G * (t + 1)) * W) >> 64 for t in range(W if count is None else count)]


def resampled(rows, seed, b):
    """the alignment of replicate b: column t is source column col(b, t)"""
    cols = columns(len(rows[0]), seed, b)
    return [bytes(r[c] for c in cols) for r in rows]


def replicate_counts(rows, seed, b):
    return R.counts(resampled(rows, seed, b))


def replicate_tree(rows, seed, b, model="kimura"):
    comp, diff = replicate_counts(rows, seed, b)
    return R.join(R.distances(comp, diff, len(rows), model))


def splits(n, joins):
    """join s -> its split: a frozenset of the two sides, each a frozenset of leaves"""
    below, out, everything = {i: frozenset([i]) for i in range(n)}, [], frozenset(range(n))
    for s in range(len(joins["join_a"])):
        L = below[int(joins["join_a"][s])] | below[int(joins["join_b"][s])]
        below[n + s] = L
        out.append(frozenset([L, everything - L]))
    return out


def support(n, main, replicates):
    """replicates: join dicts.  Returns a list over the main tree's joins"""
    mine = splits(n, main)
    assert len(set(mine)) == len(mine) == max(n - 3, 0)
    out = [0] * len(mine)
    for rep in replicates:
        theirs = set(splits(n, rep))
        for s, sp in enumerate(mine):
            out[s] += sp in theirs
    return out


def newick(names, joins, sup=None, B=0):
    """nj_ref.newick with the label of node N + s between its `)` and its `:`"""
    if not B or len(names) <= 3:
        return R.newick(names, joins)
    N = len(names)

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
                out.append(":%.6f)%d" % (joins["len_b"][s], (200 * int(sup[s]) + B) // (2 * B)))
        return "".join(out)

    return "(" + ",".join("%s:%.6f" % (sub(int(joins["root_node"][t])), joins["root_len"][t]) for t in range(3)) + ");\n"


def boot_of_fasta(text, B, seed, model="kimura"):
    """everything uc_tree_infer_boot writes: {"nwk": the labelled line, "support": [...], "boottrees": the B unlabelled lines}"""
    names, rows = R.read_fasta(text)
    comp, diff = R.counts(rows)
    main = R.join(R.distances(comp, diff, len(rows), model))
    reps = [replicate_tree(rows, seed, b, model) for b in range(B)]
    sup = support(len(rows), main, reps)
    return {"nwk": newick(names, main, sup, B), "support": sup, "boottrees": "".join(R.newick(names, r) for r in reps)}
