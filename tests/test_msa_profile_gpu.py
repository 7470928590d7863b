"""Rule UC-T/P (`unicore tree -a profile`) on the GPU: the kernels of uc_msa_profile.hip equal the host twin equal the Python reference
(msa_profile_ref.py), byte for byte, on the shared case list (msa_profile_cases.py: row counts, row lengths, widths around the column chunk,
300 groups, floor division, an asymmetric matrix with entries at +-48, ties, gap open / extend bits, unaligned and re-aligned rows, a dropped
column), over 2 and 3 rounds and under a budget of one task per launch; then uc_tree_refined and `bin/unicore tree -a profile` on the golden
database against the committed fixture tests/golden/tree_profile_d50.json and the reference."""
import json
import os
import subprocess

import numpy as np
import pytest

import msa_profile_cases as PC
import msa_profile_ref as P
import msa_ref as R
import util
from test_msa_profile import same_align, same_layout, layout_kw
from test_msa_profile import test_the_cases_hold_what_they_are_for  # noqa: F401  (collected here too: the cases the kernels run on hold their properties)

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
def material(U, O):
    """{name: (keyword set, the reference's alignment, the reference's layout)}, computed once"""
    g = U.msa_profile_geometry()
    out = {}
    for name, kw in PC.cases(O, g["chunk"], g["cap"]).items():
        a = P.align(**kw)
        out[name] = (kw, a, P.layout(**layout_kw(kw, a)))
    return out


def test_geometry_and_case_list(U, material):
    g = U.msa_profile_geometry()
    assert g["chunk"] >= 2 and g["task_bytes_per_cell"] == 1
    for W in (1, 63, 64, 65, g["chunk"] - 1, g["chunk"], g["chunk"] + 1) + ((g["cap"] - 1, g["cap"], g["cap"] + 1) if g["cap"] else ()):
        assert "width_%d" % W in material
    assert all("rows_%d" % m in material for m in (2, 3, 8)) and all("length_%d" % L in material for L in (1, 2, 63, 64, 65, 257))


@pytest.mark.parametrize("name", ["rows_2", "rows_3", "rows_8", "length_1", "length_2", "length_63", "length_64", "length_65", "length_257", "many_groups", "rounding",
                                  "asymmetric", "ties", "gap_bits", "gap_bits_open_eq_ext", "unaligned", "realigned", "empty_column_and_single"])
def test_kernels_equal_twin_equal_reference(U, material, name):
    kw, want, want_l = material[name]
    dev = U.msa_profile_align(device=-1, **kw)
    same_align(dev, want, name)
    same_align(dev, U.msa_profile_align(**kw), name)
    l = U.msa_profile_layout(device=-1, **layout_kw(kw, dev))
    same_layout(l, want_l, name)
    same_layout(l, U.msa_profile_layout(**layout_kw(kw, dev)), name)


def test_widths_around_the_chunk(U, material):
    names = [n for n in material if n.startswith("width_")]
    assert len(names) >= 7
    for name in names:
        kw, want, want_l = material[name]
        dev = U.msa_profile_align(device=-1, **kw)
        same_align(dev, want, name)
        same_layout(U.msa_profile_layout(device=-1, **layout_kw(kw, dev)), want_l, name)


@pytest.mark.parametrize("rounds", [2, 3])
def test_rounds(U, material, rounds):
    for name in ("rows_8", "empty_column_and_single", "unaligned", "width_65"):
        kw = material[name][0]
        base = {k: kw[k] for k in ("grp_off", "res_off", "res", "S3", "SA", "gap_open", "gap_ext")}
        w_ref, c_ref, _ = P.refine(width=kw["width"], cells=kw["cells"], rounds=rounds, **base)
        width, cells = kw["width"], kw["cells"]
        for _ in range(rounds):
            a = U.msa_profile_align(device=-1, width=width, cells=cells, **base)
            l = U.msa_profile_layout(device=-1, **layout_kw(dict(kw, width=width, cells=cells), a))
            width, cells = l["width"], l["cells"]
        same_layout({"width": width, "cells": cells}, {"width": w_ref, "cells": c_ref}, (name, rounds))


def test_budget_of_one_task_per_launch(U, material, monkeypatch):
    monkeypatch.setenv("UC_TREE_BUDGET_BYTES", "64")
    for name in ("rows_8", "width_129", "asymmetric", "many_groups"):
        kw, want, _ = material[name]
        same_align(U.msa_profile_align(device=-1, **kw), want, name)


def test_refusals_come_before_the_device(U, material):
    kw = material["rows_2"][0]
    bad = kw["cells"][0].copy()
    bad[0] = ord("*")
    for over in (dict(gap_open=0, gap_ext=1), dict(cells=[bad, kw["cells"][1]])):
        with pytest.raises(U.UcError) as ei:
            U.msa_profile_align(device=-1, **dict(kw, **over))
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


def test_golden_library_cli_and_host(U, O, prof, tmp_path, monkeypatch):
    db, gold = os.path.join(GOLD, "db"), json.load(open(os.path.join(GOLD, "tree_profile_d50.json")))
    star = json.load(open(os.path.join(GOLD, "tree_default_d50.json")))
    want, info = P.tree_files(O, util.oracle_params(O, R.FIXED_OPTS), db, prof[1], 50, 1)
    assert R.digest(want) == gold["rounds_1"] and gold["rounds_1"]["combined.fasta"] != star["combined.fasta"] != gold["rounds_2"]["combined.fasta"]
    monkeypatch.setenv("UC_TREE_DUMP", "1")
    st = U.tree(db, prof[0], str(tmp_path / "lib"), 50, aligner="profile")
    monkeypatch.delenv("UC_TREE_DUMP")
    got = R.read_tree(str(tmp_path / "lib"))
    tsv = {k: got.pop(k) for k in list(got) if k.endswith(("refine.tsv", "pair_scores.tsv"))}
    assert got == want
    n_rows = sum(len(v.splitlines()) for v in prof[1].values())
    assert st["refine"]["n_rounds"] == 1 and st["refine"]["n_tasks"] == n_rows and st["n_rows"] == n_rows and len(st["refine"]["width_before"]) == 1
    assert st["refine"]["width_after"][0] == st["n_columns"] and st["refine"]["n_cells"] > 0
    for gene, v in info.items():      # round, row, score, qs, ts of every row
        a = v["refine"][0]
        lines = ["1\t%d\t%d\t%d\t%d" % (r, a["score"][r], a["qs"][r], a["ts"][r]) for r in range(len(a["score"]))]
        assert tsv["fasta/%s/refine.tsv" % gene].decode().splitlines() == lines, gene
    r = cli("-n", "-a", "profile", db, prof[0], str(tmp_path / "cli"))
    assert r.returncode == 0 and r.stderr == "" and "1 refinement rounds" in r.stdout, r.stderr
    assert R.read_tree(str(tmp_path / "cli")) == want
    # two rounds; the host twins behind the same driver; one task per launch
    r = cli("-n", "-a", "profile", "--refine-iters", "2", "-v", "1", db, prof[0], str(tmp_path / "cli2"))
    assert r.returncode == 0 and R.digest(R.read_tree(str(tmp_path / "cli2"))) == gold["rounds_2"]
    monkeypatch.setenv("UC_TREE_HOST", "1")
    U.tree(db, prof[0], str(tmp_path / "host"), 50, aligner="profile", refine_iters=2)
    assert R.digest(R.read_tree(str(tmp_path / "host"))) == gold["rounds_2"]
    monkeypatch.delenv("UC_TREE_HOST")
    monkeypatch.setenv("UC_TREE_BUDGET_BYTES", "64")
    U.tree(db, prof[0], str(tmp_path / "small"), 50, aligner="profile")
    assert R.read_tree(str(tmp_path / "small")) == want


def test_star_stays_what_it_is(U, prof, tmp_path):
    """-a star, and zero rounds through the new entry point, write the star fixture"""
    import ctypes as C
    db, star = os.path.join(GOLD, "db"), json.load(open(os.path.join(GOLD, "tree_default_d50.json")))
    r = cli("-n", "-a", "star", "-v", "1", db, prof[0], str(tmp_path / "cli"))
    assert r.returncode == 0 and R.digest(R.read_tree(str(tmp_path / "cli"))) == star
    o, st = U.make_opts("", 1, 1, -1), U.UcTreeRefinedStats()
    assert U.lib().uc_tree_refined(db.encode(), prof[0].encode(), str(tmp_path / "zero").encode(), 50, b"", 0, C.byref(o), C.byref(st)) == 0
    assert R.digest(R.read_tree(str(tmp_path / "zero"))) == star and st.n_rounds == 0 and st.tree.n_groups == 11


def test_nj_after_profile(U, prof, tmp_path):
    db, gold = os.path.join(GOLD, "db"), json.load(open(os.path.join(GOLD, "tree_profile_d50.json")))
    out = str(tmp_path / "o")
    r = cli("-t", "nj", "-a", "profile", "-v", "1", db, prof[0], out)
    assert r.returncode == 0, r.stderr
    assert R.digest({k: v for k, v in R.read_tree(out).items() if k not in ("nj.nwk", "tree.chk")} | {"tree.chk": b"0"}) == gold["rounds_1"]
    assert open(os.path.join(out, "tree.chk")).read() == "1"
    nwk = open(os.path.join(out, "nj.nwk")).read()
    U.tree_infer(os.path.join(out, "combined.fasta"), str(tmp_path / "again.nwk"))
    assert nwk == open(str(tmp_path / "again.nwk")).read() and nwk.endswith(";\n")
