"""Rule UC-N/B (bootstrap support of the tree builder `nj`) on the GPU: the kernels of uc_nj_boot.hip equal their host twins equal
the plain-Python reference (nj_boot_ref.py) on the shared case list (nj_boot_cases.py) - integers equal, fp64 by their bits; then
uc_tree_infer_boot, `bin/unicore tree -t nj -p "--bootstrap 20 --seed 7"` and `bin/unicore gene-tree` on the golden database against the committed
fixture tests/golden/nj_boot.json and against the reference computed live from the files the run wrote."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nj_boot_cases as BC
import nj_boot_ref as BR
import nj_cases as NC
import nj_ref as R
import util
from test_nj_boot import bits, refusals

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


# ---- counts: device == host twin == reference
@pytest.mark.parametrize("n_index", range(6))
def test_counts(U, n_index):
    g = U.nj_geometry()
    T, C = g["tile"], g["chunk"]
    sizes = sorted({s[0] for s in BC.count_shapes(T, C)})
    assert sizes == [2, 3, T - 1, T, T + 1, 2 * T + 2]
    shapes = [s for s in BC.count_shapes(T, C) if s[0] == sizes[n_index]]
    assert [s[1] for s in shapes] == [1, 3, C - 1, C, C + 1, 2 * C + 3]
    for k, (n, w) in enumerate(shapes):
        rows = BC.shape_rows(n, w)
        for rep0, n_rep in BC.REP_SETS:
            comp, diff = U.nj_boot_counts(list(rows), BC.SEED, rep0, n_rep, device=-1)
            hc, hd = U.nj_boot_counts(list(rows), BC.SEED, rep0, n_rep, threads=4)
            assert comp.dtype == diff.dtype == np.uint32 and comp.shape == (n_rep, n * (n - 1) // 2)
            assert np.array_equal(comp, hc) and np.array_equal(diff, hd), (n, w, rep0, n_rep)
            if (rep0, n_rep) == BC.REP_SETS[k % 3]:      # the reference: the first replicate of one set per shape (plain Python, n^2 w steps each)
                rc, rd = BC.reference_counts(rows, BC.SEED, rep0)
                assert comp[0].tolist() == rc and diff[0].tolist() == rd, (n, w, rep0)


def test_counts_contents(U):
    for name, rows in BC.content_rows().items():
        for rep0, n_rep in BC.REP_SETS:
            comp, diff = U.nj_boot_counts(rows, BC.SEED, rep0, n_rep, device=-1)
            hc, hd = U.nj_boot_counts(rows, BC.SEED, rep0, n_rep)
            assert np.array_equal(comp, hc) and np.array_equal(diff, hd), (name, rep0)
            for b in range(n_rep):
                rc, rd = BC.reference_counts(tuple(rows), BC.SEED, rep0 + b)
                assert comp[b].tolist() == rc and diff[b].tolist() == rd, (name, rep0, b)


@pytest.mark.parametrize("which", range(3))
def test_counts_do_not_depend_on_the_budget(U, monkeypatch, which):
    """source slices of a chunk and of one column (twice), and batches of one replicate: the same numbers"""
    g = U.nj_geometry()
    T, C = g["tile"], g["chunk"]
    rows = BC.shape_rows(T + 1, 2 * C + 3)
    budget = ((T + 1) * C, 3 * 3, 2)[which]
    for rs in BC.REP_SETS:
        want = U.nj_boot_counts(list(rows), BC.SEED, *rs, threads=4)
        monkeypatch.setenv("UC_TREE_BUDGET_BYTES", str(budget))
        comp, diff = U.nj_boot_counts(list(rows), BC.SEED, *rs, device=-1)
        assert np.array_equal(comp, want[0]) and np.array_equal(diff, want[1]), (budget, rs)


# ---- joins: the batch on the device == uc_nj_join per replicate, by bits
def replicate_matrices(U, n, n_rep):
    rows = list(BC.replicate_alignment(n))
    comp, diff = U.nj_boot_counts(rows, BC.SEED, 0, n_rep, threads=4)
    return np.stack([U.nj_distances(comp[b], diff[b], n) for b in range(n_rep)])


@pytest.mark.parametrize("case", range(11))
def test_joins(U, case):
    L = U.nj_boot_geometry()["lds_rows"]
    sizes = BC.join_sizes(L)
    assert [s[0] for s in sizes] == [4, 5, 6, 63, 64, 65, L - 1, L, L + 1, 257, 1030] and sizes[-1][1] == 2
    n, n_rep = sizes[case]
    Ds = replicate_matrices(U, n, n_rep)
    assert any(not np.array_equal(Ds[0], Ds[b]) for b in range(1, n_rep))
    before = Ds.copy()
    got = U.nj_join_batch(Ds, device=-1)
    assert np.array_equal(bits(Ds), bits(before)), n                      # D is not modified
    for b in range(n_rep):
        NC.same_joins(BC.one_of(got, b), U.nj_join(Ds[b]), (n, b))
        if n <= 65:
            NC.same_joins(BC.one_of(got, b), R.join(Ds[b].tolist()), (n, b))


def test_joins_of_one_batch_take_different_paths(U):
    for n, (names, Ds, wants) in BC.stacked_join_cases().items():
        before = Ds.copy()
        got = U.nj_join_batch(Ds, device=-1)
        for b, name in enumerate(names):
            NC.same_joins(BC.one_of(got, b), U.nj_join(Ds[b]), name)
            NC.same_joins(BC.one_of(got, b), wants[b], name)
        assert np.array_equal(bits(Ds), bits(before)), n
    NC.same_joins(BC.one_of(U.nj_join_batch(np.stack([NC.join_cases()["equal_5"][0]] * 2), device=-1), 1), NC.EQUAL_5, "the index tie-break alone, by hand")


def test_joins_in_batches_of_one(U, monkeypatch):
    L = U.nj_boot_geometry()["lds_rows"]
    monkeypatch.setenv("UC_TREE_BUDGET_BYTES", "8")
    for n in (6, L + 1):
        Ds = replicate_matrices(U, n, 3)
        got = U.nj_join_batch(Ds, device=-1)
        for b in range(3):
            NC.same_joins(BC.one_of(got, b), U.nj_join(Ds[b]), (n, b))


def test_refusals_come_before_the_device(U):
    refusals(U, -1)
    refusals(U, 1 << 20)      # an ordinal no machine has: UC_ERR_ARGS all the same, the device is not asked for


# ---- end to end on the golden database
@pytest.fixture(scope="module")
def prof(tmp_path_factory):
    d = tmp_path_factory.mktemp("prof")
    files = json.load(open(os.path.join(GOLD, "profile_default_t80.json")))
    for k, v in files.items():
        (d / k).write_bytes(v.encode("ascii"))
    return str(d)


def cli(*args, env=None):
    return subprocess.run([UNICORE] + list(args), env=dict(os.environ, UC_ALLOW_SYNTHETIC="1", **(env or {})), capture_output=True, text=True)


def read(path):
    return open(path, encoding="latin-1").read()


def strip_labels(s):
    return re.sub(r"\)\d+:", "):", s)


def test_golden_library_and_cli(U, prof, tmp_path, monkeypatch):
    db, gold, plain = os.path.join(GOLD, "db"), json.load(open(os.path.join(GOLD, "nj_boot.json"))), json.load(open(os.path.join(GOLD, "nj_default.json")))
    B, seed = gold["bootstrap"], gold["seed"]
    assert (B, seed) == (20, 7)
    tsv = "".join("%d\t%d\n" % (s, v) for s, v in enumerate(gold["support"]))
    lib = str(tmp_path / "lib")
    U.tree(db, prof, lib, 50)
    fasta = read(lib + "/combined.fasta")
    ref = BR.boot_of_fasta(fasta, B, seed)                               # computed live from the file the run wrote
    assert (ref["nwk"], ref["support"], ref["boottrees"]) == (gold["nj.nwk"], gold["support"], gold["boottrees"])
    monkeypatch.setenv("UC_TREE_DUMP", "1")
    st = U.tree_infer(lib + "/combined.fasta", lib + "/nj.nwk", bootstrap=B, seed=seed, threads=2)
    assert read(lib + "/nj.nwk") == gold["nj.nwk"] and read(lib + "/nj.nwk.boottrees") == gold["boottrees"] and read(lib + "/nj.nwk.boot.tsv") == tsv
    assert st["n_rows"] == 5 and st["n_replicates"] == B and st["n_batches"] == 1 and st["support_sum"] == sum(gold["support"])
    assert strip_labels(gold["nj.nwk"]) == plain["nj.nwk"]                # the main tree is the plain call's, in every digit
    # B = 0 is the plain call, byte for byte
    U.tree_infer(lib + "/combined.fasta", lib + "/plain.nwk")
    assert U.lib().uc_tree_infer_boot((lib + "/combined.fasta").encode(), (lib + "/zero.nwk").encode(), None, 0, seed, None, None) == 0
    assert open(lib + "/zero.nwk", "rb").read() == open(lib + "/plain.nwk", "rb").read() == plain["nj.nwk"].encode() and not os.path.exists(lib + "/zero.nwk.boot.tsv")
    # a second seed: other replicates, the same main tree
    U.tree_infer(lib + "/combined.fasta", lib + "/s8.nwk", bootstrap=B, seed=8)
    assert read(lib + "/s8.nwk.boottrees") != gold["boottrees"] and read(lib + "/s8.nwk.boottrees") == BR.boot_of_fasta(fasta, B, 8)["boottrees"]
    assert strip_labels(read(lib + "/s8.nwk")) == plain["nj.nwk"]
    # a budget of a few columns per slice and one replicate per batch
    monkeypatch.setenv("UC_TREE_BUDGET_BYTES", "64")
    st = U.tree_infer(lib + "/combined.fasta", lib + "/small.nwk", bootstrap=B, seed=seed)
    assert st["n_batches"] == B and read(lib + "/small.nwk") == gold["nj.nwk"] and read(lib + "/small.nwk.boottrees") == gold["boottrees"]
    monkeypatch.delenv("UC_TREE_BUDGET_BYTES")
    # the host twins give the same files
    monkeypatch.setenv("UC_TREE_HOST", "1")
    U.tree_infer(lib + "/combined.fasta", lib + "/host.nwk", bootstrap=B, seed=seed)
    assert read(lib + "/host.nwk") == gold["nj.nwk"] and read(lib + "/host.nwk.boottrees") == gold["boottrees"] and read(lib + "/host.nwk.boot.tsv") == tsv
    monkeypatch.delenv("UC_TREE_HOST")
    monkeypatch.delenv("UC_TREE_DUMP")
    # the CLI: alignment, inference with labels, checkpoint; then the host twins
    out = str(tmp_path / "cli")
    r = cli("tree", "-t", "nj", "-p", "--bootstrap 20 --seed 7", db, prof, out, env={"UC_TREE_DUMP": "1"})
    assert r.returncode == 0 and r.stderr == "" and "Aligning genes 11/11... Done" in r.stdout and r.stdout.endswith("Inferring phylogenetic tree... Done\n"), r.stderr
    assert read(out + "/nj.nwk") == gold["nj.nwk"] and read(out + "/tree.chk") == "1" and read(out + "/nj.nwk.boottrees") == gold["boottrees"] and read(out + "/nj.nwk.boot.tsv") == tsv
    assert read(out + "/nj.nwk") == BR.boot_of_fasta(read(out + "/combined.fasta"), B, seed)["nwk"]
    host = str(tmp_path / "host")
    r = cli("tree", "-t", "nj", "-p", "--bootstrap=20 --seed=7", "-v", "0", db, prof, host, env={"UC_TREE_HOST": "1"})
    assert r.returncode == 0 and r.stdout == "" and read(host + "/nj.nwk") == gold["nj.nwk"] and read(host + "/tree.chk") == "1"
    assert not os.path.exists(host + "/nj.nwk.boottrees")                # no dump asked for
    # without --bootstrap: today's bytes
    r = cli("tree", "-t", "nj", db, prof, out)
    assert r.returncode == 0 and read(out + "/nj.nwk") == plain["nj.nwk"]


def test_gene_tree(U, prof, tmp_path):
    db, gold = os.path.join(GOLD, "db"), json.load(open(os.path.join(GOLD, "nj_boot.json")))
    out = str(tmp_path / "o")
    assert cli("tree", "-n", "-v", "1", db, prof, out).returncode == 0
    genes = sorted(os.listdir(out + "/fasta"))
    assert genes == sorted(gold["genes"])
    two = [g for g in genes if gold["genes"][g] is not None and re.search(r"\)\d+:", gold["genes"][g])][:2]
    assert len(two) == 2                                                  # two genes whose trees have an internal branch
    (tmp_path / "names.txt").write_text("".join(g + "\n" for g in two))
    for env in ({}, {"UC_TREE_HOST": "1"}):
        r = cli("gene-tree", "-t", "nj", "-p", "--bootstrap 20 --seed 7", "--names", str(tmp_path / "names.txt"), out, env=env)
        assert r.returncode == 0 and r.stdout.endswith("Inferring gene specific phylogenetic trees 2/2...Done\n"), r.stdout + r.stderr
        assert sorted(g for g in genes if os.path.exists("%s/fasta/%s/nj.nwk" % (out, g))) == two
        for g in two:
            path = "%s/fasta/%s/nj.nwk" % (out, g)
            assert read(path) == gold["genes"][g] == BR.boot_of_fasta(read("%s/fasta/%s/%s.fa.filtered" % (out, g, g)), 20, 7)["nwk"], g
            os.remove(path)
