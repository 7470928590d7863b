"""Rule UC-N (the tree builder `nj`) on the GPU: the kernels of uc_nj.hip equal their host twins equal the plain-Python reference
(nj_ref.py) on every case of the shared list (nj_cases.py) - integers equal, fp64 by their bits; then uc_tree + uc_tree_infer, `bin/unicore tree
-t nj` and `bin/unicore gene-tree -t nj` on the golden database against the committed fixture tests/golden/nj_default.json and against the
reference computed live from the files the run wrote."""
import json
import os
import subprocess

import numpy as np
import pytest

import msa_ref as MR
import nj_cases as NC
import nj_ref as R
import util
from test_nj import bits, refusals

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")
IQTREE_REFUSAL = ("Error: tree inference would start the external program iqtree, which this build does not do; pass -n/--no-inference and run it on "
                  "combined.fasta\n")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


# ---- kernels == host twins == reference
def test_counts(U, monkeypatch):
    g = U.nj_geometry()
    cases = NC.count_cases(g["tile"], g["chunk"])
    for name, (rows, (comp, diff)) in cases.items():
        c, d = U.nj_counts(rows, device=-1)
        hc, hd = U.nj_counts(rows)
        assert c.dtype == d.dtype == np.uint32, name
        assert np.array_equal(c, hc) and np.array_equal(d, hd) and c.tolist() == comp and d.tolist() == diff, name
    for name, (comp, diff) in NC.hand_counts().items():
        c, d = U.nj_counts(NC.hand_rows()[name], device=-1)
        assert (c.tolist(), d.tolist()) == (comp, diff), name


def test_counts_in_column_slices(U, monkeypatch):
    """a byte budget below n x w: the same counts from slices of 1, 3 and chunk columns"""
    g = U.nj_geometry()
    T, C = g["tile"], g["chunk"]
    cases = NC.count_cases(T, C)
    for name, budget in (("shape_%dx%d" % (T + 1, 2 * C + 3), (T + 1) * C), ("shape_%dx%d" % (T + 1, 2 * C + 3), (T + 1) * (C + 7)), ("shape_3x%d" % (C + 1), 3 * 3),
                         ("shape_2x5", 2), ("campaign_1", 1), ("every_byte", 3 * 100)):
        rows, (comp, diff) = cases[name]
        monkeypatch.setenv("UC_TREE_BUDGET_BYTES", str(budget))
        c, d = U.nj_counts(rows, device=-1)
        assert c.tolist() == comp and d.tolist() == diff, (name, budget)


def test_joins(U):
    for name, (D, want) in NC.join_cases().items():
        before = D.copy()
        got = U.nj_join(D, device=-1)
        NC.same_joins(got, U.nj_join(D), name)
        NC.same_joins(got, want, name)
        assert np.array_equal(bits(D), bits(before)), name
    NC.same_joins(U.nj_join(NC.join_cases()["equal_5"][0], device=-1), NC.EQUAL_5, "the index tie-break alone, by hand")
    for name, D in NC.additive_cases().items():      # independent of the reference: the joins' tree has D as its path metric, to the bit
        assert np.array_equal(NC.tree_metric(NC.edges_of_joins(len(D), U.nj_join(D, device=-1)), len(D)), D), name


def test_single_entry_across_the_route_boundary_and_on_ties(U):
    """uc_nj_join_dev is a batch of one replicate: the workgroup minimum by shuffles and the per-replicate partials of the three launches per step
    serve the main tree.  Equal to the host twin by bits, and to replicate 0 of a batch of two (the LDS kernel up to lds_rows, the same three
    launches above)"""
    L = U.nj_boot_geometry()["lds_rows"]
    cases = NC.route_cases(L)
    assert sorted({len(D) for D in cases.values()}) == [4, 5, L, L + 1, 257] and len(cases) == 15
    for name, D in cases.items():
        before = D.copy()
        got = U.nj_join(D, device=-1)
        NC.same_joins(got, U.nj_join(D), name)
        pair = U.nj_join_batch(np.stack([D, D]), device=-1)
        NC.same_joins(got, {k: v[0] for k, v in pair.items()}, name + ", replicate 0 of two")
        assert np.array_equal(bits(D), bits(before)), name


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


def test_golden_library_and_cli(U, prof, tmp_path, monkeypatch):
    db, gold, tree_gold = os.path.join(GOLD, "db"), json.load(open(os.path.join(GOLD, "nj_default.json"))), json.load(open(os.path.join(GOLD, "tree_default_d50.json")))
    lib = str(tmp_path / "lib")
    U.tree(db, prof, lib, 50)
    st = U.tree_infer(lib + "/combined.fasta", lib + "/nj.nwk")
    assert read(lib + "/combined.fasta") == tree_gold["combined.fasta"]
    assert read(lib + "/nj.nwk") == gold["nj.nwk"] == R.tree_of_fasta(read(lib + "/combined.fasta"))
    assert st["n_rows"] == 5 and st["n_columns"] == len(tree_gold["combined.fasta"].splitlines()[1])
    # the CLI: alignment, inference, checkpoint
    out = str(tmp_path / "cli")
    r = cli("tree", "-t", "nj", db, prof, out)
    assert r.returncode == 0 and r.stderr == "" and "Aligning genes 11/11... Done" in r.stdout and r.stdout.endswith("Inferring phylogenetic tree... Done\n"), r.stderr
    assert read(out + "/nj.nwk") == gold["nj.nwk"] and read(out + "/tree.chk") == "1"
    assert MR.digest(MR.read_tree(out)) == dict(tree_gold, **{"tree.chk": "1"})      # everything the alignment wrote is what `tree -n` writes
    # a second run finds combined.fasta, skips the alignment and infers again: the same bytes
    os.remove(out + "/nj.nwk")
    r = cli("tree", "-t", "nj", db, prof, out)
    assert r.returncode == 0 and r.stdout == "Concatenated alignment file %s/combined.fasta already exists, skipping alignment step\nInferring phylogenetic tree... Done\n" % out
    assert read(out + "/nj.nwk") == gold["nj.nwk"] and read(out + "/tree.chk") == "1"
    # model p and a budget of a few columns per slice
    r = cli("tree", "-t", "nj", "-p", "--model p", "-v", "1", db, prof, out, env={"UC_TREE_BUDGET_BYTES": "64"})
    assert r.returncode == 0 and r.stdout == "" and read(out + "/nj.nwk") == R.tree_of_fasta(tree_gold["combined.fasta"], "p") != gold["nj.nwk"]
    # the same with the host twins
    host = str(tmp_path / "host")
    r = cli("tree", "-t", "nj", "-v", "0", db, prof, host, env={"UC_TREE_HOST": "1"})
    assert r.returncode == 0 and r.stdout == "" and read(host + "/nj.nwk") == gold["nj.nwk"] and read(host + "/tree.chk") == "1"
    monkeypatch.setenv("UC_TREE_HOST", "1")
    U.tree_infer(lib + "/combined.fasta", lib + "/host.nwk")
    assert read(lib + "/host.nwk") == gold["nj.nwk"]
    monkeypatch.delenv("UC_TREE_HOST")
    # -n with nj: accepted, not run
    noinf = str(tmp_path / "noinf")
    r = cli("tree", "-n", "-t", "nj", db, prof, noinf)
    assert r.returncode == 0 and not os.path.exists(noinf + "/nj.nwk") and read(noinf + "/tree.chk") == "0"
    # the distances of the device run, pair by pair against the reference
    monkeypatch.setenv("UC_TREE_DUMP", "1")
    U.tree_infer(lib + "/combined.fasta", lib + "/dump.nwk")
    names, rows = R.read_fasta(read(lib + "/combined.fasta"))
    comp, diff = R.counts(rows)
    want = ["%d\t%d\t%d\t%d\t%s" % (i, j, comp[k], diff[k], "%.17g" % R.distance(comp[k], diff[k]))
            for k, (i, j) in enumerate((i, j) for i in range(len(rows)) for j in range(i + 1, len(rows)))]
    assert read(lib + "/dump.nwk.dist.tsv").splitlines() == want


def test_gene_tree(U, prof, tmp_path):
    db, gold = os.path.join(GOLD, "db"), json.load(open(os.path.join(GOLD, "nj_default.json")))
    out = str(tmp_path / "o")
    assert cli("tree", "-n", "-v", "1", db, prof, out).returncode == 0
    genes = sorted(os.listdir(out + "/fasta"))
    assert genes == sorted(gold["genes"]) and len(genes) == 11
    r = cli("gene-tree", "-t", "nj", out)
    assert r.returncode == 0 and r.stdout.endswith("Inferring gene specific phylogenetic trees 11/11...Done\n"), r.stdout + r.stderr
    n_trees = 0
    for g in genes:
        path = "%s/fasta/%s/nj.nwk" % (out, g)
        if gold["genes"][g] is None:
            assert not os.path.exists(path), g
            continue
        n_trees += 1
        assert read(path) == gold["genes"][g] == R.tree_of_fasta(read("%s/fasta/%s/%s.fa.filtered" % (out, g, g))), g
        os.remove(path)
    assert n_trees >= 2
    # --names with two genes writes exactly two
    two = [g for g in genes if gold["genes"][g] is not None][:2]
    (tmp_path / "names.txt").write_text("".join(g + "\n" for g in two))
    r = cli("gene-tree", "-t", "nj", "--names", str(tmp_path / "names.txt"), "-v", "2", out)
    assert r.returncode == 0 and r.stdout == ""
    assert sorted(g for g in genes if os.path.exists("%s/fasta/%s/nj.nwk" % (out, g))) == two
    for g in two:
        assert read("%s/fasta/%s/nj.nwk" % (out, g)) == gold["genes"][g]
    # the host twins give the same files
    r = cli("gene-tree", "-t", "nj", "-v", "1", out, env={"UC_TREE_HOST": "1"})
    assert r.returncode == 0 and all(read("%s/fasta/%s/nj.nwk" % (out, g)) == gold["genes"][g] for g in genes if gold["genes"][g] is not None)


def test_external_builders_still_refuse(prof, tmp_path):
    db, out = os.path.join(GOLD, "db"), str(tmp_path / "o")
    r = cli("tree", "-t", "iqtree", db, prof, out)
    assert r.returncode == 1 and r.stdout == "" and r.stderr == IQTREE_REFUSAL and not os.path.exists(out)
    r = cli("tree", db, prof, out)                                           # iqtree is the default
    assert r.returncode == 1 and r.stderr == IQTREE_REFUSAL and not os.path.exists(out)
