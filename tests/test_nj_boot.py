"""Rule UC-N/B (bootstrap support of the tree builder `nj`) without a GPU: the host twins (uc_nj_boot_columns / uc_nj_boot_counts /
uc_nj_join_batch / uc_nj_support / uc_nj_newick_support) against the plain-Python reference (nj_boot_ref.py) on the shared case list
(nj_boot_cases.py) - integers equal, fp64 by their bits -, every refusal, uc_tree_infer_boot and the CLI under UC_TREE_HOST=1, and the host sources
under the address and undefined-behaviour sanitizers in a program of their own (nj_boot_host_check.cpp).  The HIP kernels: test_nj_boot_gpu.py."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import nj_boot_cases as BC
import nj_boot_ref as BR
import nj_cases as NC
import nj_ref as R
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")
NEW_SYMBOLS = ("uc_nj_boot_columns", "uc_nj_boot_counts", "uc_nj_boot_counts_dev", "uc_nj_join_batch", "uc_nj_join_batch_dev", "uc_nj_support",
               "uc_nj_newick_support", "uc_nj_boot_geometry", "uc_tree_infer_boot")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- draws
def test_splitmix_known_answer():
    assert BR.mix(BR.G) == BR.MIX_G == 0xE220A8397B1DCDAF      # SplitMix64's first output from state 0
    assert BR.mix(0) == 0


def test_draws(U, tmp_path):
    for w in BC.DRAW_WIDTHS[:-1]:
        for seed in BC.DRAW_SEEDS:
            for rep in BC.DRAW_REPS:
                got = U.nj_boot_columns(w, seed, rep)
                assert got.dtype == np.uint32 and got.tolist() == BR.columns(w, seed, rep), (w, seed, rep)
                assert all(0 <= c < w for c in got.tolist())
    # replicate 0 of seed 0 draws from key mix(G): the known answer is in the chain
    assert U.nj_boot_columns(1 << 16, 0, 0)[0] == (BR.mix(BR.MIX_G + BR.G) << 16) >> 64
    # the widest alignment, the first 64 draws: the entry point writes all w (8 GiB), so the draw function of uc_nj.h - the one the entry point,
    # the host twin and the kernel call - is asked through the stand-alone program, without the sanitizers
    w = BC.DRAW_WIDTHS[-1]
    assert w == 2 ** 31 - 1
    exe = str(tmp_path / "draws")
    csrc = os.path.join(util.ROOT, "unicore_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I" + os.path.join(util.ROOT, "include"), "-I" + csrc, os.path.join(util.ROOT, "tests", "nj_boot_host_check.cpp"),
                         os.path.join(csrc, "uc_nj_host.cpp"), os.path.join(csrc, "uc_nj_boot_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    for seed in BC.DRAW_SEEDS:
        for rep in BC.DRAW_REPS:
            r = subprocess.run([exe, "draws", str(w), str(seed), str(rep), "64"], capture_output=True, text=True)
            want = BR.columns(w, seed, rep, 64)
            assert r.returncode == 0 and [int(x) for x in r.stdout.split()] == want and all(0 <= c < w for c in want) and len(set(want)) == 64, (seed, rep, r.stderr)


# ---- replicate counts
@pytest.mark.parametrize("n_index", range(6))
def test_counts(U, n_index):
    g = U.nj_geometry()
    T, C = g["tile"], g["chunk"]
    shapes = [s for s in BC.count_shapes(T, C) if s[0] == sorted({s[0] for s in BC.count_shapes(T, C)})[n_index]]
    assert len(shapes) == 6
    for k, (n, w) in enumerate(shapes):
        rows = BC.shape_rows(n, w)
        for rep0, n_rep in BC.REP_SETS:
            comp, diff = U.nj_boot_counts(list(rows), BC.SEED, rep0, n_rep, threads=1 + k % 3)
            assert comp.dtype == diff.dtype == np.uint32 and comp.shape == diff.shape == (n_rep, n * (n - 1) // 2)
            for b in range(n_rep):      # uc_nj_counts of the explicitly gathered rows: not through the new reference
                c, d = U.nj_counts(BC.gathered(rows, U.nj_boot_columns(w, BC.SEED, rep0 + b)))
                assert np.array_equal(comp[b], c) and np.array_equal(diff[b], d), (n, w, rep0, b)
            if (rep0, n_rep) == BC.REP_SETS[k % 3]:      # the reference: the first replicate of one set per shape (plain Python, n^2 w steps each)
                rc, rd = BC.reference_counts(rows, BC.SEED, rep0)
                assert comp[0].tolist() == rc and diff[0].tolist() == rd, (n, w, rep0)


def test_counts_contents(U):
    for name, rows in BC.content_rows().items():
        for rep0, n_rep in BC.REP_SETS:
            comp, diff = U.nj_boot_counts(rows, BC.SEED, rep0, n_rep, threads=2)
            for b in range(n_rep):
                rc, rd = BC.reference_counts(tuple(rows), BC.SEED, rep0 + b)
                assert comp[b].tolist() == rc and diff[b].tolist() == rd, (name, rep0, b)
    # a single column: every replicate is the original
    rows = [b"A", b"C", b"A", b"-"]
    comp, diff = U.nj_boot_counts(rows, 3, 0, 4)
    c0, d0 = U.nj_counts(rows)
    assert all(np.array_equal(comp[b], c0) and np.array_equal(diff[b], d0) for b in range(4))
    # no replicate: nothing is written
    comp, diff = U.nj_boot_counts(rows, 3, 7, 0)
    assert comp.shape == (0, 6)


# ---- batched joins
def test_join_batch(U):
    for n, (names, Ds, wants) in BC.stacked_join_cases().items():
        before = Ds.copy()
        got = U.nj_join_batch(Ds)
        assert got["join_a"].shape == (len(Ds), max(n - 3, 0)) and got["root_len"].shape == (len(Ds), 3)
        for b, name in enumerate(names):
            NC.same_joins(BC.one_of(got, b), U.nj_join(Ds[b]), name)
            NC.same_joins(BC.one_of(got, b), wants[b], name)
        assert np.array_equal(bits(Ds), bits(before)), n
    two = U.nj_join_batch(np.array([[[0, 0.75], [0.75, 0]], [[0, 2.0], [2.0, 0]]]))
    assert two["root_node"].tolist() == [[0, 1, U.NJ_NO_NODE]] * 2 and two["root_len"].tolist() == [[0.375, 0.375, 0.0], [1.0, 1.0, 0.0]]


# ---- support and the labelled line
def test_support_and_labels_by_hand(U):
    names = list("abcd")
    # B = 1, 2, 3 fix the rounding: 1/2 -> 50, 1/3 -> 33, 2/3 -> 67, 1/6 is 17 (half up from 16.67)
    for reps, want_sup in (([BC.FOUR_AB], 1), ([BC.FOUR_AC], 0), ([BC.FOUR_AB, BC.FOUR_AC], 1), ([BC.FOUR_CD, BC.FOUR_AC, BC.FOUR_AC], 1),
                           ([BC.FOUR_CD, BC.FOUR_AB, BC.FOUR_AC], 2)):
        B = len(reps)
        sup = U.nj_support(4, BC.FOUR_AB, [r["join_a"] for r in reps], [r["join_b"] for r in reps])
        assert sup.dtype == np.uint32 and sup.tolist() == [want_sup] == BR.support(4, BC.FOUR_AB, reps), reps
        line = U.nj_newick(names, BC.FOUR_AB, sup, B)
        label = {(1, 1): "100", (0, 1): "0", (1, 2): "50", (1, 3): "33", (2, 3): "67"}[(want_sup, B)]
        assert line == "((a:0.100000,b:0.200000)%s:0.050000,c:0.300000,d:0.400000);\n" % label == BR.newick(names, BC.FOUR_AB, sup, B)
    assert U.nj_newick(names, BC.FOUR_AB, [1], 6) == "((a:0.100000,b:0.200000)17:0.050000,c:0.300000,d:0.400000);\n" == BR.newick(names, BC.FOUR_AB, [1], 6)
    assert U.nj_newick(names, BC.FOUR_AB, [1], 200).count(")1:") == 1 and U.nj_newick(names, BC.FOUR_AB, [1], 201).count(")0:") == 1      # 0.5 % is the edge
    # B = 0: today's line, with or without a support array
    assert U.nj_newick(names, BC.FOUR_AB, [1], 0) == U.nj_newick(names, BC.FOUR_AB) == R.newick(names, BC.FOUR_AB)
    # N = 2 and 3: no internal branch, no support, no label
    for n in (2, 3):
        D = NC.random_matrix(random.Random(n), n)
        j = U.nj_join(D)
        assert U.nj_support(n, j, np.zeros((5, 0), np.uint32), np.zeros((5, 0), np.uint32)).tolist() == []
        assert U.nj_newick(list("abc")[:n], j, None, 5) == U.nj_newick(list("abc")[:n], j) == BR.newick(list("abc")[:n], R.join(D.tolist()), [], 5)
    # a name that needs quoting, a caterpillar of nine leaves, replicates that are other trees
    names = ["it's", "a b", "c", "d", "e", "f", "g", "h", "i"]
    main = BC.caterpillar(9)
    rng = random.Random(9)
    reps = [R.join(NC.random_matrix(rng, 9).tolist()) for _ in range(7)] + [main]
    sup = U.nj_support(9, main, [r["join_a"] for r in reps], [r["join_b"] for r in reps])
    assert sup.tolist() == BR.support(9, main, reps) and min(sup) >= 1
    line = U.nj_newick(names, main, sup, len(reps))
    assert line == BR.newick(names, main, sup, len(reps)) and line.startswith("(((((((" + "'it''s':1.000000,'a b':1.000000)")
    assert line.count(")") == 7 and line.rstrip().endswith(",h:1.000000,i:1.000000);")


def test_one_column_makes_every_label_100(U, tmp_path, monkeypatch):
    monkeypatch.setenv("UC_TREE_HOST", "1")
    text = ">a\nA\n>b\nA\n>c\nC\n>d\nC\n>e\nD\n>f\n-\n"
    (tmp_path / "in.fa").write_text(text)
    st = U.tree_infer(str(tmp_path / "in.fa"), str(tmp_path / "o.nwk"), bootstrap=11, seed=5)
    got = (tmp_path / "o.nwk").read_text()
    assert got == BR.boot_of_fasta(text, 11, 5)["nwk"] and got.count(")100:") == 3 and got.count(")") == 4
    assert st["support_min"] == 11 and st["support_sum"] == 33 and st["n_replicates"] == 11 and st["n_rows"] == 6 and set(st["seconds"]) == set(U.NJ_BOOT_PHASES)


# ---- the file level through the host twins
def golden_fasta():
    return json.load(open(os.path.join(GOLD, "tree_default_d50.json")))["combined.fasta"]


def test_tree_infer_boot_host_on_the_golden_alignment(U, tmp_path, monkeypatch):
    monkeypatch.setenv("UC_TREE_HOST", "1")
    fasta, gold = golden_fasta(), json.load(open(os.path.join(GOLD, "nj_boot.json")))
    (tmp_path / "combined.fasta").write_text(fasta)
    src = str(tmp_path / "combined.fasta")
    # B = 0 is uc_tree_infer, byte for byte
    U.tree_infer(src, str(tmp_path / "plain.nwk"))
    assert U.lib().uc_tree_infer_boot(src.encode(), str(tmp_path / "zero.nwk").encode(), None, 0, 7, None, None) == 0
    assert (tmp_path / "zero.nwk").read_bytes() == (tmp_path / "plain.nwk").read_bytes() == json.load(open(os.path.join(GOLD, "nj_default.json")))["nj.nwk"].encode()
    assert sorted(os.listdir(tmp_path)) == ["combined.fasta", "plain.nwk", "zero.nwk"]
    # B = 20, seed 7: the committed fixture and the reference computed live, with the dump files
    monkeypatch.setenv("UC_TREE_DUMP", "1")
    for threads, budget in ((1, None), (3, "200")):      # a budget of one replicate per batch: the same files
        if budget:
            monkeypatch.setenv("UC_TREE_BUDGET_BYTES", budget)
        st = U.tree_infer(src, str(tmp_path / "b.nwk"), bootstrap=gold["bootstrap"], seed=gold["seed"], threads=threads)
        ref = BR.boot_of_fasta(fasta, gold["bootstrap"], gold["seed"])
        assert (tmp_path / "b.nwk").read_text() == gold["nj.nwk"] == ref["nwk"]
        assert (tmp_path / "b.nwk.boottrees").read_text() == gold["boottrees"] == ref["boottrees"]
        assert (tmp_path / "b.nwk.boot.tsv").read_text() == "".join("%d\t%d\n" % (s, v) for s, v in enumerate(gold["support"])) and gold["support"] == ref["support"]
        assert os.path.exists(tmp_path / "b.nwk.dist.tsv")
        assert st["n_batches"] == (20 if budget else 1) and st["support_sum"] == sum(gold["support"]) and st["support_min"] == min(gold["support"])
    monkeypatch.delenv("UC_TREE_BUDGET_BYTES")
    # the labels are the only difference to the plain tree; another seed: other replicates, the same main tree
    strip = lambda s: __import__("re").sub(r"\)\d+:", "):", s)
    assert strip(gold["nj.nwk"]) == (tmp_path / "plain.nwk").read_text()
    U.tree_infer(src, str(tmp_path / "s8.nwk"), bootstrap=20, seed=8)
    assert strip((tmp_path / "s8.nwk").read_text()) == (tmp_path / "plain.nwk").read_text()
    assert (tmp_path / "s8.nwk.boottrees").read_text() != gold["boottrees"] and (tmp_path / "s8.nwk.boottrees").read_text().count("\n") == 20
    # model p
    U.tree_infer(src, str(tmp_path / "p.nwk"), "p", bootstrap=5, seed=1)
    assert (tmp_path / "p.nwk").read_text() == BR.boot_of_fasta(fasta, 5, 1, "p")["nwk"]


# ---- refusals
def refused(U, fn, *a, **kw):
    with pytest.raises(U.UcError) as ei:
        fn(*a, **kw)
    assert ei.value.code == U.UC_ERR_ARGS, (a, kw)


def refusals(U, device):
    rows = [b"ACDE", b"ACDF", b"CCDE", b"ACDA"]
    refused(U, U.nj_boot_counts, [b"ACDE"], 1, 0, 1, device=device)                       # N = 1
    refused(U, U.nj_boot_counts, [b"", b""], 1, 0, 1, device=device)                      # W = 0
    refused(U, U.nj_boot_counts, rows, 1, 100000, 1, device=device)                       # replicate 100,000 does not exist
    refused(U, U.nj_boot_counts, rows, 1, 0, 100001, device=device)
    refused(U, U.nj_join_batch, np.zeros((2, 1, 1)), device=device)
    bad = np.stack([np.ones((4, 4)) - np.eye(4)] * 3)
    bad[2, 1, 2] = 2.0                                                                   # the last replicate is not symmetric
    refused(U, U.nj_join_batch, bad, device=device)
    bad[2, 1, 2] = bad[2, 2, 1] = np.inf
    refused(U, U.nj_join_batch, bad, device=device)


def test_refusals(U, tmp_path, monkeypatch):
    refusals(U, None)
    refused(U, U.nj_boot_columns, 0, 1, 0)
    refused(U, U.nj_boot_columns, 2 ** 31, 1, 0)
    refused(U, U.nj_boot_columns, 5, 1, 100000)
    refused(U, U.nj_support, 4, dict(BC.FOUR_AB, join_b=[0]), [[0]], [[1]])               # a node joined twice
    refused(U, U.nj_support, 4, BC.FOUR_AB, [[0]], [[4]])                                 # a node before it exists
    refused(U, U.nj_newick, list("abcd"), BC.FOUR_AB, [3], 2)                             # more support than replicates
    refused(U, U.nj_newick, list("abcd"), BC.FOUR_AB, None, 2)                            # labels without support
    refused(U, U.nj_newick, list("abcd"), BC.FOUR_AB, [1], 100001)
    monkeypatch.setenv("UC_TREE_HOST", "1")
    (tmp_path / "in.fa").write_text(">a\nACDE\n>b\nACDF\n>c\nCCDE\n>d\nACDA\n")
    refused(U, U.tree_infer, str(tmp_path / "in.fa"), str(tmp_path / "o.nwk"), bootstrap=100001)
    refused(U, U.tree_infer, str(tmp_path / "in.fa"), str(tmp_path / "o.nwk"), "jc69", bootstrap=3)
    assert not os.path.exists(tmp_path / "o.nwk")
    st = U.tree_infer(str(tmp_path / "in.fa"), str(tmp_path / "o.nwk"), bootstrap=100000 // 1000, seed=2 ** 64 - 1)      # the seed's whole range
    assert st["n_replicates"] == 100


# ---- the CLI
def cli(*args, env=None):
    return subprocess.run([UNICORE] + list(args), env=dict(os.environ, UC_ALLOW_SYNTHETIC="1", **(env or {})), capture_output=True, text=True)


def test_cli_parser(tmp_path):
    db, prof, out = os.path.join(GOLD, "db"), str(tmp_path / "prof"), str(tmp_path / "o")
    for cmd in ("tree", "gene-tree"):
        r = cli(cmd, "-h")
        assert r.returncode == 0 and "--bootstrap" in r.stdout and "--seed" in r.stdout and "--model kimura|p" in r.stdout
    for opts, word in (("--bootstrap", "--bootstrap"), ("--bootstrap x", "x"), ("--bootstrap -1", "-1"), ("--bootstrap 100001", "100001"), ("--bootstrap=1e3", "1e3"),
                       ("--bootstrap 10 --seed", "--seed"), ("--seed 18446744073709551616", "18446744073709551616"), ("--seed=-3", "-3"), ("--bootstrap 3 extra", "extra"),
                       ("--bootstrap= --seed 1", "--bootstrap")):
        r = cli("tree", "-t", "nj", "-p", opts, db, prof, out)
        assert r.returncode == 1 and word in r.stderr and not os.path.exists(out), (opts, r.stderr)
        r = cli("tree", "-n", "-t", "nj", "-p", opts, db, prof, out)                      # refused with -n too: the word is wrong either way
        assert r.returncode == 1 and word in r.stderr and not os.path.exists(out), (opts, r.stderr)
    # -n: parsed and not run
    os.makedirs(out)
    open(os.path.join(out, "combined.fasta"), "w").write(">x\nAC\n>y\nAD\n>z\nCC\n>w\nCD\n")
    r = cli("tree", "-n", "-t", "nj", "-p", "--bootstrap=100000 --seed=18446744073709551615 --model p", db, prof, out)
    assert r.returncode == 0 and sorted(os.listdir(out)) == ["combined.fasta"]
    os.makedirs(os.path.join(out, "fasta", "g1"))
    r = cli("gene-tree", "-t", "nj", "-p", "--bootstrap many", out)
    assert r.returncode == 1 and "many" in r.stderr and os.listdir(os.path.join(out, "fasta", "g1")) == []


def test_cli_bootstrap_with_the_host_twins(tmp_path):
    out = tmp_path / "o"
    (out / "fasta" / "gA").mkdir(parents=True)
    (out / "fasta" / "gB").mkdir()
    rows = NC.evolved_rows(random.Random(77), 8, 60)
    text = BC.fasta_of(["t%d" % i for i in range(8)], rows)
    small = ">x\nAC\n>y\nAD\n>z\nCC\n"                                                   # three rows: no internal branch, no label
    (out / "combined.fasta").write_text(text)
    (out / "fasta" / "gA" / "gA.fa.filtered").write_text(text)
    (out / "fasta" / "gB" / "gB.fa.filtered").write_text(small)
    env = {"UC_TREE_HOST": "1"}
    db, none = os.path.join(GOLD, "db"), str(tmp_path / "none")
    r = cli("tree", "-t", "nj", db, none, str(out), env=env)
    plain = (out / "nj.nwk").read_bytes()
    assert r.returncode == 0 and plain.decode() == R.tree_of_fasta(text)
    for opts in ("--seed 5", "--bootstrap 0", "--bootstrap=0 --seed=9"):                 # --seed without --bootstrap: accepted and unused
        r = cli("tree", "-t", "nj", "-p", opts, db, none, str(out), env=env)
        assert r.returncode == 0 and r.stderr == "" and (out / "nj.nwk").read_bytes() == plain and sorted(os.listdir(out)) == ["combined.fasta", "fasta", "nj.nwk", "tree.chk"]
    r = cli("tree", "-t", "nj", "-p", "--bootstrap 12 --seed 3", "-c", "2", db, none, str(out), env=dict(env, UC_TREE_DUMP="1"))
    ref = BR.boot_of_fasta(text, 12, 3)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout == "Concatenated alignment file %s/combined.fasta already exists, skipping alignment step\nInferring phylogenetic tree... Done\n" % out
    assert (out / "nj.nwk").read_text() == ref["nwk"] != plain.decode() and (out / "tree.chk").read_text() == "1"
    assert (out / "nj.nwk.boottrees").read_text() == ref["boottrees"]
    assert (out / "nj.nwk.boot.tsv").read_text() == "".join("%d\t%d\n" % (s, v) for s, v in enumerate(ref["support"]))
    # the default seed is 1
    r = cli("tree", "-t", "nj", "-p", "--bootstrap=12", db, none, str(out), env=env)
    assert r.returncode == 0 and (out / "nj.nwk").read_text() == BR.boot_of_fasta(text, 12, 1)["nwk"]
    # gene-tree: every gene under the same seed
    r = cli("gene-tree", "-t", "nj", "-p", "--bootstrap 12 --seed 3 --model p", str(out), env=env)
    assert r.returncode == 0 and r.stdout.endswith("\nInferring gene specific phylogenetic trees 2/2...Done\n"), r.stdout + r.stderr
    assert (out / "fasta" / "gA" / "nj.nwk").read_text() == BR.boot_of_fasta(text, 12, 3, "p")["nwk"]
    assert (out / "fasta" / "gB" / "nj.nwk").read_text() == R.tree_of_fasta(small, "p")


def test_header_binding_and_abi(U):
    hdr = open(os.path.join(util.ROOT, "include", "unicore_cluster.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in hdr and name in U.SYMBOLS and hasattr(U.lib(), name), name
    assert "#define UC_ABI_VERSION 9" in hdr and U.ABI_VERSION == 9 and U.lib().uc_abi_version() == 9
    assert "#define UC_NJ_BOOT_NPHASE 7" in hdr and len(U.NJ_BOOT_PHASES) == 7 and "#define UC_NJ_NPHASE 5" in hdr
    assert U.nj_boot_geometry()["lds_rows"] >= 64


# ---- the host sources under the sanitizers, in a program of their own
def test_host_twins_under_sanitizers(tmp_path):
    csrc = os.path.join(util.ROOT, "unicore_amd", "csrc")
    exe = str(tmp_path / "nj_boot_host_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-pthread",
                         "-I" + os.path.join(util.ROOT, "include"), "-I" + csrc, os.path.join(util.ROOT, "tests", "nj_boot_host_check.cpp"),
                         os.path.join(csrc, "uc_nj_host.cpp"), os.path.join(csrc, "uc_nj_boot_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    assert run.stdout.strip() == "nj_boot_host_check: ok"
