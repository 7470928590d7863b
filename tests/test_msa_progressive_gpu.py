"""Rule UC-T/G (`unicore tree -a progressive`) on the GPU: the kernels of uc_msa_progressive.hip equal the host twin equal the Python reference
(msa_progressive_ref.py), byte for byte, on the shared case list (msa_progressive_cases.py: widths around the column chunk crossed, row counts with a
floor division that rounds a negative quotient, 300 merges in one call, an asymmetric matrix with entries at +-48, ties, gap open = extend, all-negative
scores, overhangs, a side of width 0, every letter the checks accept), under a budget of one task per launch, along forced caterpillar and balanced merge lists; the guide trees on the
device; then uc_tree_progressive and `bin/unicore tree -n -a progressive` on the golden database against tests/golden/tree_progressive_d50.json."""
import json
import os
import subprocess

import numpy as np
import pytest

import msa_progressive_cases as GC
import msa_progressive_ref as G
import msa_ref as R
import util
from test_msa_progressive import same_merge, same_msa, ref_merges
from test_msa_progressive import test_the_cases_hold_what_they_are_for  # noqa: F401  (collected here too: the cases the kernels run on hold their properties)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.fixture(scope="module")
def merges():
    return {name: (kw, ref_merges(kw)) for name, kw in GC.merge_cases().items()}


@pytest.fixture(scope="module")
def trees():
    return {name: (kw, G.progressive(**kw)) for name, kw in GC.progressive_cases().items()}


@pytest.mark.parametrize("name", ["widths", "rows_1_1", "rows_1_2", "rows_3_5", "rows_40_60", "many", "asymmetric", "asymmetric_swapped", "ties", "open_eq_ext", "all_negative",
                                  "overhangs", "width_0", "letters"])
def test_kernels_equal_twin_equal_reference(U, merges, name):
    kw, want = merges[name]
    dev = U.msa_merge(device=-1, **kw)
    same_merge(dev, want, name)
    same_merge(dev, U.msa_merge(**kw), name)


def test_budget_of_one_task_per_launch(U, merges, trees, monkeypatch):
    monkeypatch.setenv("UC_TREE_BUDGET_BYTES", "64")
    for name in ("widths", "rows_3_5", "width_0", "ties"):
        same_merge(U.msa_merge(device=-1, **merges[name][0]), merges[name][1], name)
    kw, want = trees["several_groups"]
    got = U.msa_progressive(device=-1, **kw)
    same_msa(got, want, "several_groups")
    assert got["stats"]["n_launches"] == 5 * got["stats"]["n_merges"]


@pytest.mark.parametrize("m", GC.TREE_ROWS)
def test_forced_trees(U, trees, m):
    for shape in ("caterpillar", "balanced"):
        kw, want = trees["%s_%d" % (shape, m)]
        got = U.msa_progressive(device=-1, **kw)
        same_msa(got, want, (shape, m))
        same_msa(got, U.msa_progressive(**kw), (shape, m))
        levels = m - 1 if shape == "caterpillar" else int(np.ceil(np.log2(m)))
        assert got["stats"]["n_levels"] == levels and got["stats"]["n_merges"] == m - 1 and got["stats"]["n_launches"] == 5 * levels


def test_several_groups_share_their_levels(U, trees):
    kw, want = trees["several_groups"]
    got = U.msa_progressive(device=-1, **kw)
    same_msa(got, want, "several_groups")
    assert got["stats"]["n_levels"] == 4 and got["stats"]["n_launches"] == 20      # the caterpillar of 5 rows sets the depth


def test_limits_hold_on_the_widths_not_on_the_leaf_sums(U):
    """1000 rows of 100 residues, balanced: the sums of the leaves' lengths break the width limits, the widths do not; the device runs it and equals the twin"""
    m, L, kw = GC.leaf_sum_case()
    ml = [np.array(G.balanced(m), np.uint32)]
    got = U.msa_progressive(device=-1, merges=ml, **kw)
    same_msa(got, U.msa_progressive(merges=ml, threads=16, **kw), "1000 x 100")
    assert L <= int(got["width"][0]) < 2 * L and got["stats"]["n_levels"] == 10


def test_guide_on_the_device(U):
    for name, (go, tri, selfs) in GC.guide_cases(big=True).items():
        dev, host = U.msa_guide(go, tri, selfs, device=-1), U.msa_guide(go, tri, selfs)
        t0 = 0
        for g in range(len(go) - 1):
            b, m = int(go[g]), int(go[g + 1] - go[g])
            assert dev["D"][g].tobytes() == host["D"][g].tobytes() and np.array_equal(dev["merges"][g], host["merges"][g]), (name, g)
            assert G.check_merges(m, [tuple(int(v) for v in p) for p in dev["merges"][g]])
            if m <= 24:      # the reference's join is cubic in plain Python
                D, ml = G.guide(tri[t0:t0 + m * (m - 1) // 2], selfs[b:b + m])
                assert dev["D"][g].tobytes() == np.array(D, np.float64).reshape(m, m).tobytes() and [tuple(int(v) for v in p) for p in dev["merges"][g]] == ml, (name, g)
            t0 += m * (m - 1) // 2


def test_refusals_come_before_the_device(U, merges):
    kw = merges["rows_1_2"][0]
    bad = [c.copy() for c in kw["a"]]
    bad[0][0] = ord("*")
    for over in (dict(gap_open=0, gap_ext=1), dict(a=bad)):
        with pytest.raises(U.UcError) as ei:
            U.msa_merge(device=-1, **dict(kw, **over))
        assert ei.value.code == U.UC_ERR_ARGS


# ---- end to end on the golden database
@pytest.fixture(scope="module")
def prof(tmp_path_factory):
    d = tmp_path_factory.mktemp("prof")
    files = json.load(open(os.path.join(GOLD, "profile_default_t80.json")))
    for k, v in files.items():
        (d / k).write_bytes(v.encode("ascii"))
    return str(d), {k: v.encode("ascii") for k, v in files.items() if k.endswith(".txt")}


def cli(*args, env=None):
    return subprocess.run([UNICORE, "tree"] + list(args), env=dict(os.environ, UC_ALLOW_SYNTHETIC="1", **(env or {})), capture_output=True, text=True)


def test_golden_library_cli_and_host(U, prof, tmp_path, monkeypatch):
    db, gold = os.path.join(GOLD, "db"), json.load(open(os.path.join(GOLD, "tree_progressive_d50.json")))
    star = json.load(open(os.path.join(GOLD, "tree_default_d50.json")))
    assert gold["combined.fasta"] != star["combined.fasta"]
    monkeypatch.setenv("UC_TREE_DUMP", "1")
    st = U.tree(db, prof[0], str(tmp_path / "lib"), 50, aligner="progressive")
    monkeypatch.delenv("UC_TREE_DUMP")
    got = R.read_tree(str(tmp_path / "lib"))
    tsv = {k: got.pop(k) for k in list(got) if k.endswith(("guide.tsv", "pair_scores.tsv"))}
    assert R.digest(got) == gold
    n_rows = sum(len(v.splitlines()) for v in prof[1].values())
    pg = st["progressive"]
    assert st["n_rows"] == n_rows and pg["n_groups_aligned"] == 11 and pg["n_merges"] == n_rows - 11 and st["n_rows_unaligned"] == 0
    assert pg["n_launches"] == 5 * pg["n_levels"] and pg["n_cells"] > 0 and pg["width_before"] == st["n_columns"] and pg["width_after"] == st["n_columns_kept"]
    for gene in (k[:-4] for k in prof[1]):      # the dump: D as %.17g, then the merge list, which is a tree over the gene's rows
        m = len(prof[1][gene + ".txt"].splitlines())
        lines = tsv["fasta/%s/guide.tsv" % gene].decode().splitlines()
        d = [l.split("\t") for l in lines if l.startswith("#D")]
        ml = [tuple(int(x) for x in l.split("\t")[1:]) for l in lines if not l.startswith("#D")]
        assert len(d) == m * (m - 1) // 2 and all(0.0 <= float(x[3]) <= 1.0 and repr(float(x[3])) == repr(float("%.17g" % float(x[3]))) for x in d)
        assert G.check_merges(m, ml), gene
    r = cli("-n", "-a", "progressive", db, prof[0], str(tmp_path / "cli"))
    assert r.returncode == 0 and r.stderr == "" and "progressive MSA: %d merges" % (n_rows - 11) in r.stdout, r.stderr
    assert R.digest(R.read_tree(str(tmp_path / "cli"))) == gold
    # the host twins behind the same driver; one task per launch
    monkeypatch.setenv("UC_TREE_HOST", "1")
    U.tree(db, prof[0], str(tmp_path / "host"), 50, aligner="progressive")
    assert R.read_tree(str(tmp_path / "host")) == got
    monkeypatch.delenv("UC_TREE_HOST")
    monkeypatch.setenv("UC_TREE_BUDGET_BYTES", "64")
    U.tree(db, prof[0], str(tmp_path / "small"), 50, aligner="progressive")
    assert R.read_tree(str(tmp_path / "small")) == got


def test_star_and_profile_stay_what_they_are(prof, tmp_path):
    db = os.path.join(GOLD, "db")
    r = cli("-n", "-a", "star", "-v", "1", db, prof[0], str(tmp_path / "star"))
    assert r.returncode == 0 and R.digest(R.read_tree(str(tmp_path / "star"))) == json.load(open(os.path.join(GOLD, "tree_default_d50.json")))
    r = cli("-n", "-a", "profile", "-v", "1", db, prof[0], str(tmp_path / "profile"))
    assert r.returncode == 0 and R.digest(R.read_tree(str(tmp_path / "profile"))) == json.load(open(os.path.join(GOLD, "tree_profile_d50.json")))["rounds_1"]


def test_nj_after_progressive(U, prof, tmp_path):
    db, gold = os.path.join(GOLD, "db"), json.load(open(os.path.join(GOLD, "tree_progressive_d50.json")))
    out = str(tmp_path / "o")
    r = cli("-t", "nj", "-a", "progressive", "-v", "1", db, prof[0], out)
    assert r.returncode == 0, r.stderr
    assert R.digest({k: v for k, v in R.read_tree(out).items() if k not in ("nj.nwk", "tree.chk")} | {"tree.chk": b"0"}) == gold
    assert open(os.path.join(out, "tree.chk")).read() == "1"
    nwk = open(os.path.join(out, "nj.nwk")).read()
    U.tree_infer(os.path.join(out, "combined.fasta"), str(tmp_path / "again.nwk"))
    assert nwk == open(str(tmp_path / "again.nwk")).read() and nwk.endswith(";\n")
