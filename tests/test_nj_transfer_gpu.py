"""Rule UC-N/T (transfer bootstrap support of the tree builder `nj`) on the GPU: the kernels of uc_nj_transfer.hip equal the host
twin equal the plain-Python reference (nj_transfer_ref.py) on the shared tree shapes (nj_transfer_cases.py), at the smallest sizes where the kernels
can go wrong - one and two splits, the word edges, a partial tile of splits whose padded rows must not count as splits, the edges of the word chunk -
and with a budget of one replicate per launch; then uc_tree_infer_support and `bin/unicore tree|gene-tree -p "--support tbe"` on the golden database
against the committed fixture tests/golden/nj_transfer.json and against the reference computed live from the files the run wrote."""
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import nj_boot_cases as BC
import nj_cases as NC
import nj_transfer_cases as TC
import nj_transfer_ref as TR
import util
from test_nj_transfer import refusals

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


def sizes(U):
    g = U.nj_transfer_geometry()
    T, C = g["tile"], g["chunk"]
    return [4, 5, 32, 33, 64, 65, T - 1 + 3, T + 3, T + 1 + 3, 2 * T + 1 + 3, 32 * C - 1, 32 * C, 32 * C + 1]


def check(U, n, main, reps, want=None):
    ra, rb = TC.arrays(reps)
    phi, light = U.nj_transfer(n, main, ra, rb, device=-1)
    hphi, hlight = U.nj_transfer(n, main, ra, rb, threads=4)
    assert phi.dtype == light.dtype == np.uint32 and phi.shape == (len(reps), n - 3) and light.shape == (n - 3,)
    assert np.array_equal(light, hlight) and np.array_equal(phi, hphi), n
    assert (phi <= light - 1).all() and np.array_equal((phi == 0).sum(0), U.nj_support(n, main, ra, rb)), n
    if want is not None:
        assert phi.tolist() == want[0] and light.tolist() == want[1], n
    return phi


@pytest.mark.parametrize("k", range(13))
def test_device_twin_reference(U, k):
    n = sizes(U)[k]
    main, reps = TC.case(n)
    assert len(reps) == 6
    phi = check(U, n, main, reps, TC.reference(n))
    assert (phi[0] == 0).all() and phi[1].max() <= 1 and phi[5].max() <= 1      # the copy and the two regrafts
    if n > 8:
        assert phi[2].max() > 1                                                 # the unrelated tree


@pytest.mark.parametrize("shape", ("caterpillar", "balanced", "random"))
def test_partial_tile_with_deep_splits(U, shape):
    """N - 3 = tile - 1, tile + 1 and 2 tile + 1: the last tile of splits is padded with all-zero rows.  A zero row taken for a split would be at
    distance light from a main split; against replicates of another shape the deep splits of a caterpillar or a balanced tree have no nearer one"""
    T = U.nj_transfer_geometry()["tile"]
    for n in (T - 1 + 3, T + 1 + 3, 2 * T + 1 + 3):
        main, reps = TC.shaped_case(n, shape)
        want = TR.transfer(n, main, reps)
        phi = check(U, n, main, reps, want)
        assert (phi[-1] == 0).all()
        if shape != "random":
            assert (phi[:3].min(0) >= 4).any(), "a split that is far from every split of three replicates"


def test_batches_do_not_change_a_byte(U, monkeypatch):
    g = U.nj_transfer_geometry()
    n = g["tile"] + 1 + 3
    main, reps = TC.case(n, 8)
    want = check(U, n, main, reps)
    for budget in ("1", "40000"):      # one replicate per launch; a few
        monkeypatch.setenv("UC_TREE_BUDGET_BYTES", budget)
        assert np.array_equal(check(U, n, main, reps), want), budget


def test_refusals_come_before_the_device(U):
    refusals(U, -1)
    refusals(U, 1 << 20)      # an ordinal no machine has: UC_ERR_ARGS all the same, the device is not asked for


# ---- end to end on the golden alignment and database
def cli(*args, env=None):
    return subprocess.run([UNICORE] + list(args), env=dict(os.environ, UC_ALLOW_SYNTHETIC="1", **(env or {})), capture_output=True, text=True)


def read(path):
    return open(path, encoding="latin-1").read()


def test_tree_infer_tbe_on_the_device(U, tmp_path, monkeypatch):
    gold = json.load(open(os.path.join(GOLD, "nj_transfer.json")))
    fasta = json.load(open(os.path.join(GOLD, "tree_default_d50.json")))["combined.fasta"]
    (tmp_path / "combined.fasta").write_text(fasta)
    src = str(tmp_path / "combined.fasta")
    monkeypatch.setenv("UC_TREE_DUMP", "1")
    assert gold["bootstrap"] == 12
    st = U.tree_infer(src, str(tmp_path / "dev.nwk"), bootstrap=12, seed=gold["seed"], support="tbe", threads=2)
    monkeypatch.setenv("UC_TREE_HOST", "1")
    hs = U.tree_infer(src, str(tmp_path / "host.nwk"), bootstrap=12, seed=gold["seed"], support="tbe", threads=2)
    g12 = gold
    for name in ("dev", "host"):
        assert read(str(tmp_path / name) + ".nwk") == g12["nj.nwk"] and read(str(tmp_path / name) + ".nwk.boot.tsv") == g12["boot.tsv"], name
        assert read(str(tmp_path / name) + ".nwk.boottrees") == g12["boottrees"], name
    assert st["support_sum"] == hs["support_sum"] == sum(g12["support"]) and st["support_min"] == min(g12["support"]) and st["n_replicates"] == 12
    # a larger alignment than the golden one: eight rows evolved along a tree, device against host against the reference
    text = BC.fasta_of(["t%d" % i for i in range(9)], NC.evolved_rows(random.Random(78), 9, 80, rate=0.3))
    (tmp_path / "nine.fa").write_text(text)
    ref = TR.transfer_of_fasta(text, 12, 3)
    monkeypatch.delenv("UC_TREE_HOST")
    U.tree_infer(str(tmp_path / "nine.fa"), str(tmp_path / "nine.nwk"), bootstrap=12, seed=3, support="tbe")
    assert read(str(tmp_path / "nine.nwk")) == ref["nwk"] and read(str(tmp_path / "nine.nwk.boot.tsv")) == ref["tsv"]
    # above host_leaves the driver's transfer phase runs the kernels (up to there the twin, also on a device run): the same files as the host run
    n = U.nj_transfer_geometry()["host_leaves"] + 2
    big = BC.fasta_of(["t%d" % i for i in range(n)], NC.evolved_rows(random.Random(79), n, 48, rate=0.3))
    (tmp_path / "big.fa").write_text(big)
    ds = U.tree_infer(str(tmp_path / "big.fa"), str(tmp_path / "bigdev.nwk"), bootstrap=4, seed=3, support="tbe", threads=2)
    monkeypatch.setenv("UC_TREE_HOST", "1")
    hs = U.tree_infer(str(tmp_path / "big.fa"), str(tmp_path / "bighost.nwk"), bootstrap=4, seed=3, support="tbe", threads=2)
    monkeypatch.delenv("UC_TREE_HOST")
    for ext in ("", ".boot.tsv", ".boottrees"):
        assert read(str(tmp_path / "bigdev.nwk") + ext) == read(str(tmp_path / "bighost.nwk") + ext), ext
    assert ds["support_sum"] == hs["support_sum"] and len(set(re.findall(r"\)(\d+):", read(str(tmp_path / "bigdev.nwk"))))) > 2      # labels of more than two kinds
    # fbp is the old call
    U.tree_infer(src, str(tmp_path / "fbp.nwk"), bootstrap=12, seed=gold["seed"], support="fbp")
    U.tree_infer(src, str(tmp_path / "old.nwk"), bootstrap=12, seed=gold["seed"])
    assert read(str(tmp_path / "fbp.nwk")) == read(str(tmp_path / "old.nwk")) and read(str(tmp_path / "fbp.nwk.boot.tsv")) == read(str(tmp_path / "old.nwk.boot.tsv"))


def test_cli_tree_and_gene_tree(U, tmp_path):
    gold = json.load(open(os.path.join(GOLD, "nj_transfer.json")))
    db = os.path.join(GOLD, "db")
    prof = tmp_path / "prof"
    prof.mkdir()
    for k, v in json.load(open(os.path.join(GOLD, "profile_default_t80.json"))).items():
        (prof / k).write_bytes(v.encode("ascii"))
    out = str(tmp_path / "o")
    r = cli("tree", "-t", "nj", "-p", "--bootstrap %d --seed %d --support tbe" % (gold["bootstrap"], gold["seed"]), db, str(prof), out, env={"UC_TREE_DUMP": "1"})
    assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith("Inferring phylogenetic tree... Done\n"), r.stderr
    assert read(out + "/nj.nwk") == gold["nj.nwk"] and read(out + "/nj.nwk.boot.tsv") == gold["boot.tsv"] and read(out + "/tree.chk") == "1"
    assert read(out + "/nj.nwk") == TR.transfer_of_fasta(read(out + "/combined.fasta"), gold["bootstrap"], gold["seed"])["nwk"]
    genes = [g for g in sorted(gold["genes"]) if gold["genes"][g] is not None and re.search(r"\)\d+:", gold["genes"][g])][:2]
    assert len(genes) == 2                                                       # two genes whose trees have an internal branch
    (tmp_path / "names.txt").write_text("".join(g + "\n" for g in genes))
    r = cli("gene-tree", "-t", "nj", "-p", "--bootstrap=%d --seed=%d --support=tbe" % (gold["bootstrap"], gold["seed"]), "--names", str(tmp_path / "names.txt"), out)
    assert r.returncode == 0 and r.stdout.endswith("Inferring gene specific phylogenetic trees 2/2...Done\n"), r.stdout + r.stderr
    for g in genes:
        assert read("%s/fasta/%s/nj.nwk" % (out, g)) == gold["genes"][g], g
