"""Rule UC-N in plain Python: integer loops for the counts, math.log per element for the transform, Python floats for the joins
(an IEEE double operation each, no fsum, nothing fused), and the Newick writer.  Names and arithmetic follow the rule line for line; the library's
host twins and HIP kernels are compared against this bit for bit."""
import math

CAP = 5.0
NO_NODE = 0xFFFFFFFF


def informative(c):
    """a cell (an int 0 .. 255): an ASCII letter other than X / x"""
    return (65 <= c <= 90 or 97 <= c <= 122) and c not in (88, 120)


def counts(rows):
    """rows: equally long bytes.  Returns (comp, diff): lists over the packed upper triangle, (i, j) with i < j in row-major order."""
    n = len(rows)
    fold = [bytes(r).upper() for r in rows]       # ASCII letters fold case; no other byte becomes a letter
    info = [[informative(c) for c in r] for r in fold]
    comp, diff = [], []
    for i in range(n):
        for j in range(i + 1, n):
            c = d = 0
            a, b, ia, ib = fold[i], fold[j], info[i], info[j]
            for x in range(len(a)):
                if ia[x] and ib[x]:
                    c += 1
                    if a[x] != b[x]:
                        d += 1
            comp.append(c)
            diff.append(d)
    return comp, diff


def distance(comp, diff, model="kimura"):
    if comp == 0:
        return CAP
    p = diff / comp
    if model == "p":
        return p
    assert model == "kimura", model
    t = 1.0 - p - 0.2 * p * p
    if t <= 0.0:
        return CAP
    d = min(CAP, -math.log(t))
    return 0.0 if d == 0.0 else d                  # -log(1) is -0.0: stored as +0.0


def distances(comp, diff, n, model="kimura"):
    """the full symmetric matrix as a list of lists"""
    D = [[0.0] * n for _ in range(n)]
    k = 0
    for i in range(n):
        for j in range(i + 1, n):
            D[i][j] = D[j][i] = distance(comp[k], diff[k], model)
            k += 1
    return D


def join(D):
    """UC-N/J.  Returns a dict: join_a, join_b, len_a, len_b (n - 3 each), root_node [3], root_len [3]."""
    N = len(D)
    assert N >= 2
    if N == 2:
        return {"join_a": [], "join_b": [], "len_a": [], "len_b": [], "root_node": [0, 1, NO_NODE], "root_len": [0.5 * D[0][1], 0.5 * D[0][1], 0.0]}
    d = [[float(x) for x in row] for row in D]
    active = [True] * N
    node = list(range(N))
    n = N
    r = [0.0] * N
    out = {"join_a": [], "join_b": [], "len_a": [], "len_b": []}
    s = 0
    while n > 3:
        act = [i for i in range(N) if active[i]]   # ascending
        for i in act:
            acc, di = 0.0, d[i]
            for k in act:
                if k != i:
                    acc = acc + di[k]
            r[i] = acc
        best = None
        for x, i in enumerate(act):
            for j in act[x + 1:]:
                q = (((n - 2) * d[i][j]) - r[i]) - r[j]
                if best is None or (q, i, j) < best:
                    best = (q, i, j)
        _, i, j = best
        dij = d[i][j]
        li = 0.5 * dij + (r[i] - r[j]) / (2 * (n - 2))
        lj = dij - li
        if not li > 0:
            li, lj = 0.0, (dij if dij > 0 else 0.0)    # a reduced distance of a matrix that is no tree metric can be negative itself
        elif not lj > 0:
            lj, li = 0.0, (dij if dij > 0 else 0.0)
        out["join_a"].append(node[i]); out["join_b"].append(node[j]); out["len_a"].append(li); out["len_b"].append(lj)
        for k in range(N):
            if active[k] and k != i and k != j:
                d[i][k] = d[k][i] = 0.5 * ((d[i][k] + d[j][k]) - dij)
        node[i] = N + s
        active[j] = False
        n -= 1
        s += 1
    a, b, c = [i for i in range(N) if active[i]]
    la = 0.5 * ((d[a][b] + d[a][c]) - d[b][c])
    lb = 0.5 * ((d[a][b] + d[b][c]) - d[a][c])
    lc = 0.5 * ((d[a][c] + d[b][c]) - d[a][b])
    out["root_node"] = [node[a], node[b], node[c]]
    out["root_len"] = [x if x > 0 else 0.0 for x in (la, lb, lc)]
    return out


def quote(name):
    if name == "" or any(ch in "()[]:;,'" or ch.isspace() for ch in name):
        return "'" + name.replace("'", "''") + "'"
    return name


def newick(names, joins):
    """one line with its newline; children in record order"""
    N = len(names)

    def sub(v):                                    # iterative: a caterpillar is N deep
        out, stack = [], [(v, 0)]
        while stack:
            x, st = stack.pop()
            if x < N:
                out.append(quote(names[x]))
                continue
            s = x - N
            if st == 0:
                out.append("(")
                stack.append((x, 1)); stack.append((joins["join_a"][s], 0))
            elif st == 1:
                out.append(":%.6f," % joins["len_a"][s])
                stack.append((x, 2)); stack.append((joins["join_b"][s], 0))
            else:
                out.append(":%.6f)" % joins["len_b"][s])
        return "".join(out)

    kids = 2 if N == 2 else 3
    return "(" + ",".join("%s:%.6f" % (sub(int(joins["root_node"][t])), joins["root_len"][t]) for t in range(kids)) + ");\n"


def read_fasta(text):
    """names up to the first white space, rows with any wrapping"""
    names, rows = [], []
    for line in text.splitlines():
        if line.startswith(">"):
            names.append(line[1:].split()[0] if line[1:].split() else "")
            rows.append([])
        elif rows:
            rows[-1].append("".join(line.split()))
    return names, ["".join(r).encode("latin-1") for r in rows]


def tree_of_fasta(text, model="kimura"):
    names, rows = read_fasta(text)
    comp, diff = counts(rows)
    return newick(names, join(distances(comp, diff, len(rows), model)))
