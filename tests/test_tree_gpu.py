"""Rule UC-T (`unicore tree --no-inference`) on the GPU: the kernels of uc_msa.hip equal their host twins equal the Python reference (msa_ref.py)
on every output array of the shared case list (tree_cases.py); then uc_tree and `bin/unicore tree -n` on the golden database against the
committed fixture tests/golden/tree_default_d50.json and against the reference over the CPU oracle, byte for byte."""
import json
import os
import subprocess

import numpy as np
import pytest

import msa_ref as R
import tree_cases as TC
import util
from test_tree import campaign, same_filter, same_star

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


# ---- kernels == host twins == reference
def test_star_hand_cases(U):
    for name, (_, case) in TC.hand_cases().items():
        dev, host = U.msa_star(device=-1, **case), U.msa_star(**case)
        same_star(dev, host, name)
        same_star(dev, R.star(**case), name)
    r = U.msa_star(device=-1, **TC.empty_case())
    assert len(r["width"]) == len(r["col"]) == len(r["cnt"]) == 0 and all(len(c) == 0 for c in r["cells"])
    _, case = TC.hand_cases()["insert_70_in_300"]
    one = U.msa_star(device=-1, **dict(case, res=case["res"][1]))
    assert len(one["cells"]) == 1 and np.array_equal(one["cells"][0], R.star(**case)["cells"][1])


def test_star_campaign(U):
    tot = {}
    for seed, groups, case in campaign():
        dev = U.msa_star(device=-1, **case)
        same_star(dev, U.msa_star(**case), seed)
        same_star(dev, R.star(**case), seed)
        for k, v in TC.events(groups).items():
            tot[k] = tot.get(k, 0) + v
    assert all(v >= 1 for v in tot.values()) and tot == dict(shared_unequal=168, trailing=183, unaligned=148, qs_positive=428)


def test_center(U):
    for name, (go, sc, want) in TC.centre_cases().items():
        got = U.msa_center(go, sc, device=-1)
        assert np.array_equal(got, U.msa_center(go, sc)) and np.array_equal(got, R.center(go, sc)), name
        if want is not None:
            assert got.tolist() == want, name


def test_filter(U):
    for name, (go, w, cells, thr, want) in TC.filter_cases().items():
        got = U.msa_filter(go, w, cells, thr, device=-1)
        same_filter(got, U.msa_filter(go, w, cells, thr), name)
        same_filter(got, R.filter(go, w, cells, thr), name)
        if want is not None:
            assert got["fwidth"].tolist() == want, name
    # every threshold on the 200 rendered groups
    _, case = TC.hand_cases()["groups_200"]
    s = U.msa_star(device=-1, **case)
    for thr in (0, 1, 50, 99, 100):
        same_filter(U.msa_filter(case["grp_off"], s["width"], s["cells"][0], thr, device=-1), R.filter(case["grp_off"], s["width"], s["cells"][0], thr), thr)


def test_refusals_come_before_the_device(U):
    _, ok = TC.hand_cases()["two_rows"]
    for kw in (dict(centre=[2]), dict(runs=[5 << 2 | 0, 2 << 2 | 3, 7 << 2 | 0]), dict(runs=[5 << 2 | 0, 2 << 2 | 2, 8 << 2 | 0]), dict(run_off=[0, 3, 2])):
        with pytest.raises(U.UcError) as ei:
            U.msa_star(device=-1, **dict(ok, **kw))
        assert ei.value.code == U.UC_ERR_ARGS, kw
    with pytest.raises(U.UcError) as ei:
        U.msa_filter([0, 1], [1], np.frombuffer(b"A", np.uint8), 101, device=-1)
    assert ei.value.code == U.UC_ERR_ARGS


# ---- end to end on the golden database
@pytest.fixture(scope="module")
def prof(tmp_path_factory):
    d = tmp_path_factory.mktemp("prof")
    files = json.load(open(os.path.join(GOLD, "profile_default_t80.json")))
    for k, v in files.items():
        (d / k).write_bytes(v.encode("ascii"))      # the gene files, copiness.tsv and profile.chk: a profile output directory as it is
    return str(d), {k: v.encode("ascii") for k, v in files.items() if k.endswith(".txt")}


@pytest.fixture(scope="module")
def reference(O, prof):
    """threshold -> (files, info) of the reference under the fixed options, computed once"""
    db, cache = os.path.join(GOLD, "db"), {}

    def get(threshold, opts=""):
        key = (threshold, opts)
        if key not in cache:
            cache[key] = R.tree_files(O, util.oracle_params(O, (R.FIXED_OPTS + " " + opts).strip()), db, prof[1], threshold)
        return cache[key]
    return get


def cli(*args, env=None):
    return subprocess.run([UNICORE, "tree"] + list(args), env=dict(os.environ, UC_ALLOW_SYNTHETIC="1", **(env or {})), capture_output=True, text=True)


def test_golden_library_and_cli(U, prof, reference, tmp_path, monkeypatch):
    db, gold = os.path.join(GOLD, "db"), json.load(open(os.path.join(GOLD, "tree_default_d50.json")))
    st = U.tree(db, prof[0], str(tmp_path / "lib"), 50)
    got = R.read_tree(str(tmp_path / "lib"))
    assert R.digest(got) == gold and got == reference(50)[0]
    assert st["n_groups"] == 11 and st["n_rows"] == sum(len(v.splitlines()) for v in prof[1].values()) and st["n_groups_dropped"] == 0
    assert st["n_pairs_scored"] == sum(len(v["scores"]) for v in reference(50)[1].values()) and st["n_rows_unaligned"] == 0
    assert st["n_columns_kept"] == len(gold["combined.fasta"].splitlines()[1]) <= st["n_columns"]
    r = cli("-n", db, prof[0], str(tmp_path / "cli"))
    assert r.returncode == 0 and r.stderr == "" and "Aligning genes 11/11... Done" in r.stdout, r.stderr
    assert R.read_tree(str(tmp_path / "cli")) == got
    # the host twins behind the same driver, and batches of a few pairs / a few cells
    monkeypatch.setenv("UC_TREE_HOST", "1")
    U.tree(db, prof[0], str(tmp_path / "host"), 50)
    assert R.read_tree(str(tmp_path / "host")) == got
    monkeypatch.delenv("UC_TREE_HOST")
    monkeypatch.setenv("UC_TREE_BUDGET_BYTES", "2048")
    U.tree(db, prof[0], str(tmp_path / "small"), 50)
    assert R.read_tree(str(tmp_path / "small")) == got
    r = cli("-n", "-v", "0", db, prof[0], str(tmp_path / "cli_host"), env={"UC_TREE_HOST": "1"})
    assert r.returncode == 0 and r.stdout == "" and R.read_tree(str(tmp_path / "cli_host")) == got


@pytest.mark.parametrize("threshold", [0, 100])
def test_thresholds_0_and_100(U, prof, reference, tmp_path, threshold, monkeypatch):
    db = os.path.join(GOLD, "db")
    want = reference(threshold)[0]
    U.tree(db, prof[0], str(tmp_path / "lib"), threshold)
    assert R.read_tree(str(tmp_path / "lib")) == want
    r = cli("-n", "-d", str(threshold), "-v", "1", db, prof[0], str(tmp_path / "cli"))
    assert r.returncode == 0 and R.read_tree(str(tmp_path / "cli")) == want
    monkeypatch.setenv("UC_TREE_HOST", "1")
    U.tree(db, prof[0], str(tmp_path / "host"), threshold)
    assert R.read_tree(str(tmp_path / "host")) == want
    if threshold == 0:      # nothing is filtered: the filtered file is the alignment
        assert all(want[k] == want[k[:-len(".filtered")]] for k in want if k.endswith(".filtered"))
    else:
        assert len(want["combined.fasta"]) < len(reference(0)[0]["combined.fasta"])


def test_aligner_options_reach_the_gapped_stage(U, prof, reference, tmp_path):
    db = os.path.join(GOLD, "db")
    want, base = reference(50, "--gap-open 12")[0], reference(50)[0]
    assert any(want[k] != base[k] for k in want if k.endswith(".fa"))
    U.tree(db, prof[0], str(tmp_path / "lib"), 50, "--gap-open 12")
    assert R.read_tree(str(tmp_path / "lib")) == want
    r = cli("-n", "-o", "--gap-open 12", "-v", "1", db, prof[0], str(tmp_path / "cli"))
    assert r.returncode == 0 and R.read_tree(str(tmp_path / "cli")) == want
    r = cli("-n", "-o", "--no-such-flag", "-v", "1", db, prof[0], str(tmp_path / "bad"))
    assert r.returncode == 1 and "--no-such-flag" in r.stderr and not os.path.exists(str(tmp_path / "bad"))


def test_second_run_rewrites_nothing(U, prof, tmp_path):
    db, out = os.path.join(GOLD, "db"), str(tmp_path / "o")
    U.tree(db, prof[0], out, 50)
    first = R.read_tree(out)
    stamp = {k: os.stat(os.path.join(out, k)).st_mtime_ns for k in first}
    st = U.tree(db, prof[0], out, 0, "--gap-open 12")       # other settings would give other files
    assert st["n_groups"] == 0 and R.read_tree(out) == first
    assert {k: os.stat(os.path.join(out, k)).st_mtime_ns for k in first} == stamp
    r = cli("-n", "-d", "0", db, prof[0], out)
    assert r.returncode == 0 and "already exists, skipping alignment step" in r.stdout and R.read_tree(out) == first


def test_centre_from_real_scores(U, prof, reference, tmp_path, monkeypatch):
    """the packed triangle the driver built, pair by pair against the oracle's sw, on three genes; and the centre it chose from it"""
    monkeypatch.setenv("UC_TREE_DUMP", "1")
    out = str(tmp_path / "o")
    U.tree(os.path.join(GOLD, "db"), prof[0], out, 50)
    info = reference(50)[1]
    for gene in sorted(info)[:3]:
        lines = open(os.path.join(out, "fasta", gene, "pair_scores.tsv")).read().splitlines()
        assert lines[0] == "#centre\t%d" % info[gene]["centre"]
        rows = [tuple(int(x) for x in l.split("\t")) for l in lines[1:]]
        m = 1 + max(j for _, j, _ in rows)
        assert [(i, j) for i, j, _ in rows] == [(i, j) for i in range(m) for j in range(i + 1, m)]
        assert [s for _, _, s in rows] == info[gene]["scores"] and len(rows) >= 3
