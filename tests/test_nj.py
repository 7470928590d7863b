"""Rule UC-N (the tree builder `nj`) without a GPU: the host twins (uc_nj_counts / uc_nj_distances / uc_nj_join / uc_nj_newick)
against the plain-Python reference (nj_ref.py) on the shared case list (nj_cases.py) - integers equal, fp64 by their bits -, every refusal,
uc_tree_infer under UC_TREE_HOST=1 against the committed fixture tests/golden/nj_default.json, the CLI's parser, and the host twins under the
address and undefined-behaviour sanitizers in a program of their own (nj_host_check.cpp).  The HIP kernels: test_nj_gpu.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import nj_cases as NC
import nj_ref as R
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- host twins == reference
def test_counts(U):
    g = U.nj_geometry()
    assert g["tile"] >= 4 and g["chunk"] >= 4
    cases = NC.count_cases(g["tile"], g["chunk"])
    assert len(cases) == 48 + len(NC.hand_rows()) + 6
    for name, (rows, (comp, diff)) in cases.items():
        for threads in (1, 3):
            c, d = U.nj_counts(rows, threads=threads)
            assert c.dtype == d.dtype == np.uint32 and c.tolist() == comp and d.tolist() == diff, name
    for name, (comp, diff) in NC.hand_counts().items():
        c, d = U.nj_counts(NC.hand_rows()[name])
        assert (c.tolist(), d.tolist()) == (comp, diff), name
    # the last column alone: a dropped tail would call the two rows identical
    for n, w in NC.count_shapes(g["tile"], g["chunk"]):
        if w >= 2:
            rows, (comp, diff) = cases["shape_%dx%d" % (n, w)]
            assert diff[0] == (1 if R.informative(rows[0][-1]) and rows[0][-1:].upper() != rows[1][-1:] else 0), (n, w)
    # a 2-D array is what a list of rows is
    rows = cases["campaign_0"][0]
    c, d = U.nj_counts(np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1))
    assert c.tolist() == cases["campaign_0"][1][0] and d.tolist() == cases["campaign_0"][1][1]


def test_distances(U):
    for name, (comp, diff, n) in NC.distance_cases().items():
        for model in ("kimura", "p"):
            D = U.nj_distances(comp, diff, n, model)
            want = np.array(R.distances(comp, diff, n, model))
            assert D.shape == (n, n) and np.array_equal(bits(D), bits(want)), (name, model)
    comp, diff, n = NC.distance_cases()["edges"]
    D = U.nj_distances(comp, diff, n)
    tri = [D[i, j] for i in range(n) for j in range(i + 1, n)]
    assert tri[0] == 5.0                                                 # nothing compares
    assert tri[1] == 0.0 and not np.signbit(tri[1])                      # -log(1) is stored as +0.0
    assert tri[2] == 5.0                                                 # p = 1: t < 0
    assert tri[3] == 5.0 and tri[4] == 5.0                               # 0.8541: t = 2.6e-6 > 0, -log t = 12.8, capped; 0.8542: t < 0
    assert tri[5] < tri[6] < 5.0 and tri[7] == 5.0 and tri[8] == 5.0     # the cap itself: -log t crosses 5 between 0.8490 and 0.8491
    assert 1.0 - 0.8541 - 0.2 * 0.8541 * 0.8541 > 0.0 > 1.0 - 0.8542 - 0.2 * 0.8542 * 0.8542
    assert tri[14] == 0.0 and 0.0 < tri[13] < 5.0
    P = U.nj_distances(comp, diff, n, "p")
    assert P[0, 1] == 5.0 and P[0, 2] == 0.0 and P[0, 3] == 1.0 and P[0, 4] == 0.8541 and np.array_equal(P, P.T) and not P.diagonal().any()


def test_joins(U):
    cases = NC.join_cases()
    assert {"random_%d" % n for n in (2, 3, 4, 5, 64, 65, 200)} <= set(cases)
    for name, (D, want) in cases.items():
        before = D.copy()
        got = U.nj_join(D)
        NC.same_joins(got, want, name)
        assert np.array_equal(bits(D), bits(before)), name                # D is not modified
        n = len(D)
        assert len(got["join_a"]) == max(n - 3, 0)
        for k in ("len_a", "len_b", "root_len"):
            assert not np.signbit(got[k]).any() and (got[k] >= 0).all(), (name, k)
    NC.same_joins(U.nj_join(cases["equal_5"][0]), NC.EQUAL_5, "the index tie-break alone, by hand")
    assert U.nj_join(cases["clamp"][0])["len_a"][0] == 0.0 and U.nj_join(cases["clamp"][0])["len_b"][0] == 0.1
    two = U.nj_join(np.array([[0, 0.75], [0.75, 0]]))
    assert two["root_node"].tolist() == [0, 1, U.NJ_NO_NODE] and two["root_len"].tolist() == [0.375, 0.375, 0.0]


def test_additive_trees_are_recovered_exactly(U):
    """edge lengths are multiples of 1/8, so every operation of the rule is exact: the tree the joins describe has the input as its path
    metric, to the bit, and a tree metric with positive edges has one tree.  Checked without the reference."""
    for name, D in NC.additive_cases().items():
        n = len(D)
        j = U.nj_join(D)
        edges = NC.edges_of_joins(n, j)
        assert all(l * 16 == int(l * 16) for _, _, l in edges), name         # two leaves hang at half of their k / 8
        assert np.array_equal(NC.tree_metric(edges, n), D), name
        inner = [l for u, v, l in edges if u >= n and v >= n]
        assert all(l > 0 for l in inner) or n == 2, name                  # no edge of the true tree collapsed


def test_newick(U):
    names = NC.NEWICK_NAMES
    D = NC.random_matrix(__import__("random").Random(11), len(names))
    j = U.nj_join(D)
    got = U.nj_newick(names, j)
    assert got == R.newick(names, R.join(D.tolist())) and got.endswith(");\n") and got.count("\n") == 1
    for quoted in ("'with space':", "'a:b':", "'it''s':", "'(paren)':", "'semi;colon':", "'comma,':", "'[brack]':", "'tab\there':"):
        assert quoted in got, quoted
    assert "plain:" in got and "Homo_sapiens.1:" in got and "'plain'" not in got
    for name, (D, want) in NC.join_cases().items():
        if len(D) <= 65:
            nm = ["s%d" % i for i in range(len(D))]
            assert U.nj_newick(nm, want) == R.newick(nm, want), name
    assert U.nj_newick(["a", "b"], R.join([[0, 1.0], [1.0, 0]])) == "(a:0.500000,b:0.500000);\n"
    five = U.nj_newick(list("abcde"), NC.EQUAL_5)
    assert five == "(((a:0.500000,b:0.500000):0.000000,c:0.500000):0.000000,d:0.500000,e:0.500000);\n"
    bad = dict(NC.EQUAL_5, join_b=[1, 1])                                 # a node joined twice
    with pytest.raises(U.UcError) as ei:
        U.nj_newick(list("abcde"), bad)
    assert ei.value.code == U.UC_ERR_ARGS


# ---- refusals
def refused(U, fn, *a, **kw):
    with pytest.raises(U.UcError) as ei:
        fn(*a, **kw)
    assert ei.value.code == U.UC_ERR_ARGS, (a, kw)


def refusals(U, device):
    refused(U, U.nj_counts, [b"ACDE"], device=device)                                   # N = 1
    refused(U, U.nj_counts, np.full((16385, 1), 65, np.uint8), device=device)           # N = 16385
    refused(U, U.nj_counts, [b"", b""], device=device)                                  # W = 0
    with pytest.raises(ValueError):
        U.nj_counts([b"ACDE", b"ACD"], device=device)                                   # ragged rows: no array to hand over
    refused(U, U.nj_join, np.zeros((1, 1)), device=device)
    refused(U, U.nj_join, np.array([[0, 1.0], [2.0, 0]]), device=device)                # not symmetric
    refused(U, U.nj_join, np.array([[0, -1.0], [-1.0, 0]]), device=device)
    refused(U, U.nj_join, np.array([[0, np.nan], [np.nan, 0]]), device=device)
    refused(U, U.nj_join, np.array([[1.0, 1.0], [1.0, 0]]), device=device)              # d(i, i) = 0


def test_refusals(U, tmp_path, monkeypatch):
    refusals(U, None)
    refused(U, U.nj_distances, [1], [0], 2, "jc69")                                     # an unknown model
    refused(U, U.nj_distances, [1], [2], 2)                                             # diff > comp
    refused(U, U.nj_distances, [], [], 1)
    monkeypatch.setenv("UC_TREE_HOST", "1")
    out = str(tmp_path / "t.nwk")

    def infer(text, model="kimura"):
        (tmp_path / "in.fa").write_bytes(text)
        return U.tree_infer(str(tmp_path / "in.fa"), out, model)

    refused(U, infer, b">a\nACDE\n")                                                    # N = 1
    refused(U, infer, b">a\nACDE\n>b\nACD\n")                                           # ragged rows
    refused(U, infer, b">a\n>b\n")                                                      # W = 0
    refused(U, infer, b">a\nACDE\n>b\nACDF\n", "jc69")
    for text in (b">a\nACDE\n>a\nACDF\n", b">\nACDE\n>b\nACDF\n", b"ACDE\n>a\nACDE\n>b\nACDF\n"):
        with pytest.raises(U.UcError) as ei:
            infer(text)
        assert ei.value.code == U.UC_ERR_IO, text
    with pytest.raises(U.UcError) as ei:
        U.tree_infer(str(tmp_path / "missing.fa"), out)
    assert ei.value.code == U.UC_ERR_IO and not os.path.exists(out)


# ---- the file level through the host twins
def test_tree_infer_host_on_the_golden_alignment(U, tmp_path, monkeypatch):
    monkeypatch.setenv("UC_TREE_HOST", "1")
    fasta = json.load(open(os.path.join(GOLD, "tree_default_d50.json")))["combined.fasta"]
    gold = json.load(open(os.path.join(GOLD, "nj_default.json")))
    (tmp_path / "combined.fasta").write_text(fasta)
    st = U.tree_infer(str(tmp_path / "combined.fasta"), str(tmp_path / "nj.nwk"))
    got = (tmp_path / "nj.nwk").read_text()
    assert got == gold["nj.nwk"] == R.tree_of_fasta(fasta)
    assert st["n_rows"] == 5 and st["n_columns"] == len(fasta.splitlines()[1]) and st["n_pairs_incomparable"] == 0 and set(st["seconds"]) == set(U.NJ_PHASES)
    assert len(gold["genes"]) == 11 and all(v is None or v.endswith(");\n") for v in gold["genes"].values())
    # wrapped lines, a description behind the name, CRLF: the same tree; model p: the reference's other tree
    names, rows = R.read_fasta(fasta)
    wrapped = "".join(">%s some description\r\n%s\r\n" % (nm, "\r\n".join(r.decode()[k:k + 60] for k in range(0, len(r), 60))) for nm, r in zip(names, rows))
    (tmp_path / "wrapped.fasta").write_bytes(wrapped.encode())
    U.tree_infer(str(tmp_path / "wrapped.fasta"), str(tmp_path / "w.nwk"))
    assert (tmp_path / "w.nwk").read_text() == got
    U.tree_infer(str(tmp_path / "combined.fasta"), str(tmp_path / "p.nwk"), "p")
    assert (tmp_path / "p.nwk").read_text() == R.tree_of_fasta(fasta, "p") != got
    # the dump: every pair with the reference's counts and the distance to 17 digits
    monkeypatch.setenv("UC_TREE_DUMP", "1")
    U.tree_infer(str(tmp_path / "combined.fasta"), str(tmp_path / "d.nwk"))
    comp, diff = R.counts(rows)
    lines = (tmp_path / "d.nwk.dist.tsv").read_text().splitlines()
    want = ["%d\t%d\t%d\t%d\t%s" % (i, j, comp[k], diff[k], "%.17g" % R.distance(comp[k], diff[k]))
            for k, (i, j) in enumerate((i, j) for i in range(5) for j in range(i + 1, 5))]
    assert lines == want


def test_clamps_and_caps_are_counted(U, tmp_path, monkeypatch):
    monkeypatch.setenv("UC_TREE_HOST", "1")
    (tmp_path / "in.fa").write_bytes(b">a\nACDEFGHIKL\n>b\nACDEFGHIKL\n>c\n----------\n>d\nCDEFGHIKLM\n")
    st = U.tree_infer(str(tmp_path / "in.fa"), str(tmp_path / "o.nwk"))
    assert st["n_pairs_incomparable"] == 3 and st["n_pairs_capped"] == 5 and st["n_lengths_clamped"] >= 2      # a and b are one point
    assert (tmp_path / "o.nwk").read_text() == R.tree_of_fasta((tmp_path / "in.fa").read_text())


# ---- the CLI's parser
def cli(*args):
    return subprocess.run([UNICORE] + list(args), env=dict(os.environ, UC_ALLOW_SYNTHETIC="1"), capture_output=True, text=True)


def test_cli_parser(tmp_path):
    db, prof, out = os.path.join(GOLD, "db"), str(tmp_path / "prof"), str(tmp_path / "o")
    r = cli("tree", "-h")
    assert r.returncode == 0 and "nj" in r.stdout and "--model kimura|p" in r.stdout and "nj.nwk" in r.stdout
    for opts in ("--nope", "--model jc69", "--model", "--model kimura extra"):
        r = cli("tree", "-t", "nj", "-p", opts, db, prof, out)
        assert r.returncode == 1 and opts.split()[-1] in r.stderr and not os.path.exists(out), (opts, r.stderr)
    r = cli("tree", "-t", "nj", "-p", "--nope", "-n", db, prof, out)          # refused by name with -n too: the word is wrong either way
    assert r.returncode == 1 and "--nope" in r.stderr
    r = cli("tree", "-t", "iqtree", db, prof, out)                           # the external builders answer as they did
    assert r.returncode == 1 and not os.path.exists(out)
    assert r.stderr == ("Error: tree inference would start the external program iqtree, which this build does not do; pass -n/--no-inference and run it on "
                        "combined.fasta\n")
    assert cli("tree", "-n", "-t", "phyml", db, prof, out).stderr == "Error: Unrecognized tree builder\n"
    # -n with nj: accepted and not run (an existing concatenation: the reference's message, no tree)
    os.makedirs(out)
    open(os.path.join(out, "combined.fasta"), "w").write(">x\nAC\n>y\nAD\n>z\nCC\n")
    r = cli("tree", "-n", "-t", "nj", "-p", "--model p", db, prof, out)
    assert r.returncode == 0 and "already exists, skipping alignment step" in r.stdout and sorted(os.listdir(out)) == ["combined.fasta"]
    # gene-tree
    r = cli("gene-tree", "-h")
    assert r.returncode == 0 and "Usage: unicore gene-tree" in r.stdout and "nj" in r.stdout
    r = cli("gene-tree")
    assert r.returncode == 0x30
    r = cli("gene-tree", "-t", "nj", str(tmp_path / "missing"))
    assert r.returncode == 1 and r.stderr == "Error: Input directory does not exist\n"
    r = cli("gene-tree", "-t", "nj", out)                                    # a directory without fasta/
    assert r.returncode == 1 and r.stderr == "Error: Input directory does not contain core structure fasta directories\n"
    os.makedirs(os.path.join(out, "fasta", "g1"))
    r = cli("gene-tree", "-t", "nj", "--realign", out)
    assert r.returncode == 1 and "--realign" in r.stderr and os.listdir(os.path.join(out, "fasta", "g1")) == []
    for b in ("iqtree", "fasttree", "raxml-ng"):
        r = cli("gene-tree", "-t", b, out)
        assert r.returncode == 1 and "external program " + b in r.stderr
    assert cli("gene-tree", out).returncode == 1                             # the default builder is iqtree
    assert cli("gene-tree", "-t", "phyml", out).stderr == "Error: Unrecognized tree builder\n"
    r = cli("gene-tree", "-t", "nj", "-p", "--nope", out)
    assert r.returncode == 1 and "--nope" in r.stderr
    for bad in (["-t"], ["-t", "nj"], ["-t", "nj", out, "extra"], ["-t", "nj", "--what", out], ["-t", "nj", "-v", "7", out]):
        r = cli("gene-tree", *bad)
        assert r.returncode == 2 and r.stderr.startswith("error: "), bad


def test_cli_infers_on_an_existing_concatenation_with_the_host_twins(tmp_path):
    """`tree -t nj` with combined.fasta present skips the alignment and infers; gene-tree walks fasta/ in byte order, warns and skips"""
    out = tmp_path / "o"
    (out / "fasta" / "gB").mkdir(parents=True)
    (out / "fasta" / "gA").mkdir()
    (out / "fasta" / "gC").mkdir()
    (out / "fasta" / "gD").mkdir()
    text = ">x\nACDEFGHIKL\n>y name\nACDEFGHIKM\n>z\nCCDEFGHIKL\n>w\nCCDEFGHIKA\n"
    (out / "combined.fasta").write_text(text)
    (out / "fasta" / "gA" / "gA.fa.filtered").write_text(text)
    (out / "fasta" / "gB" / "gB.fa.filtered").write_text(">x\nAC\n>y\nAD\n")
    (out / "fasta" / "gC" / "gC.fa.filtered").write_text(">x\nAC\n")          # one row; gD has no filtered file
    env = dict(os.environ, UC_ALLOW_SYNTHETIC="1", UC_TREE_HOST="1")
    r = subprocess.run([UNICORE, "tree", "-t", "nj", os.path.join(GOLD, "db"), str(tmp_path / "none"), str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout == "Concatenated alignment file %s/combined.fasta already exists, skipping alignment step\nInferring phylogenetic tree... Done\n" % out
    assert (out / "nj.nwk").read_text() == R.tree_of_fasta(text) and (out / "tree.chk").read_text() == "1"
    r = subprocess.run([UNICORE, "tree", "-t", "nj", "-p", "--model p", "-v", "2", os.path.join(GOLD, "db"), str(tmp_path / "none"), str(out)], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "" and (out / "nj.nwk").read_text() == R.tree_of_fasta(text, "p")
    r = subprocess.run([UNICORE, "gene-tree", "-t", "nj", str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("\nInferring gene specific phylogenetic trees 4/4...Done\n"), r.stdout      # text mode reads the \r as \n
    assert r.stdout.startswith("\nInferring gene specific phylogenetic trees 0/4...") and "gC" in r.stderr and "gD" in r.stderr
    assert (out / "fasta" / "gA" / "nj.nwk").read_text() == R.tree_of_fasta(text)
    assert (out / "fasta" / "gB" / "nj.nwk").read_text() == R.tree_of_fasta(">x\nAC\n>y\nAD\n")
    assert not (out / "fasta" / "gC" / "nj.nwk").exists() and not (out / "fasta" / "gD" / "nj.nwk").exists()
    (tmp_path / "names.txt").write_text("gB\nnot_a_gene\n")
    os.remove(out / "fasta" / "gA" / "nj.nwk"); os.remove(out / "fasta" / "gB" / "nj.nwk")
    r = subprocess.run([UNICORE, "gene-tree", "-t", "nj", "--names", str(tmp_path / "names.txt"), "-v", "1", str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "" and (out / "fasta" / "gB" / "nj.nwk").exists() and not (out / "fasta" / "gA" / "nj.nwk").exists()
    (tmp_path / "names.txt").write_text("nothing\n")
    r = subprocess.run([UNICORE, "gene-tree", "-t", "nj", "--names", str(tmp_path / "names.txt"), str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr == "Error: No gene names matched\n"


def test_header_binding_and_abi(U):
    hdr = open(os.path.join(util.ROOT, "include", "unicore_cluster.h")).read()
    for name in ("uc_nj_counts", "uc_nj_counts_dev", "uc_nj_distances", "uc_nj_join", "uc_nj_join_dev", "uc_nj_newick", "uc_nj_geometry", "uc_tree_infer"):
        assert "int %s(" % name in hdr and name in U.SYMBOLS and hasattr(U.lib(), name), name
    assert "#define UC_ABI_VERSION 9" in hdr and U.ABI_VERSION == 9 and U.lib().uc_abi_version() == 9
    assert "#define UC_NJ_NPHASE 5" in hdr and len(U.NJ_PHASES) == 5


# ---- the host twins under the sanitizers, in a program of their own
def test_host_twins_under_sanitizers(tmp_path):
    csrc = os.path.join(util.ROOT, "unicore_amd", "csrc")
    exe = str(tmp_path / "nj_host_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-pthread",
                         "-I" + os.path.join(util.ROOT, "include"), "-I" + csrc, os.path.join(util.ROOT, "tests", "nj_host_check.cpp"),
                         os.path.join(csrc, "uc_nj_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    assert run.stdout.strip() == "nj_host_check: ok"
